"""Test helper: ONNX files written by torch's own TorchScript exporter - a writer that shares nothing with onnx_import.py or
tests/helpers/onnx_write.py (the graph is serialised by torch's C++ code from its own copy of onnx.proto).

The exporter imports the ``onnx`` package only in its last post-processing step, ``onnx_proto_utils._add_onnxscript_fn``
(it looks for onnxscript functions to embed; a plain nn.Module has none).  ``export`` swaps that step for the identity while
it runs, so no ``onnx`` / ``onnxruntime`` package is needed and nothing is fetched.  The dynamo exporter (``dynamo=True``)
needs ``onnxscript`` and is not used.

A failed export raises: the calling test fails with the exporter's message, it is never skipped."""
import contextlib
import warnings

import torch


@contextlib.contextmanager
def _identity_post_step():
    """replace the exporter's onnxscript post-processing (the only user of the ``onnx`` package) by the identity; restored on exit.
    Where this torch has no such attribute the exporter runs unpatched."""
    try:
        from torch.onnx._internal.torchscript_exporter import onnx_proto_utils as mod
    except ImportError:
        mod = None
    name = "_add_onnxscript_fn"
    if mod is None or not hasattr(mod, name):
        yield
        return
    saved = getattr(mod, name)
    setattr(mod, name, lambda proto, custom_opsets: proto)
    try:
        yield
    finally:
        setattr(mod, name, saved)


def export(module, example, path, **exporter_kwargs):
    """torch.onnx.export(module, example, path, dynamo=False, **exporter_kwargs); -> str(path).  ``example``: a tensor or a
    tuple of tensors.  The module is exported as it stands (put it in eval mode first)."""
    args = example if isinstance(example, tuple) else (example,)
    with _identity_post_step(), warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        warnings.simplefilter("ignore", FutureWarning)
        warnings.simplefilter("ignore", UserWarning)
        warnings.simplefilter("ignore", torch.jit.TracerWarning)
        with torch.no_grad():
            torch.onnx.export(module, args, str(path), dynamo=False, **exporter_kwargs)
    return str(path)
