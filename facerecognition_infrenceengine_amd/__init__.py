"""MI355X-native detect -> align -> embed -> match engine (HIP C-ABI + Python host)."""
__version__ = "0.1.0"

from .face_analysis import Face, FaceAnalysis, FaceEngine  # noqa: E402,F401
from .activity import ActivityGate  # noqa: E402,F401
from .tracks import FaceTracks  # noqa: E402,F401
from .quality import FaceQuality  # noqa: E402,F401
from .hud import Hud  # noqa: E402,F401
from .redact import Redactor  # noqa: E402,F401
from .chips import FaceChips  # noqa: E402,F401
from .jpeg import JpegEncoder  # noqa: E402,F401
from .jpeg_decode import JpegDecoder  # noqa: E402,F401
from .gallery import DuplicateOverflowError, DuplicatePairs, GalleryMatcher  # noqa: E402,F401
