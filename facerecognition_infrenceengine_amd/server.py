"""The four HTTP routes of /root/reference/infrenceServer.py:685-724, byte-compatible JSON and
status codes, as an app factory with the managers injected (the reference builds module-level
singletons that connect to a database at import: :682-683) - and two routes the reference has no
counterpart for (it shows its frames with cv2.imshow, :648-667): the latest processed frame of a
camera as a JPEG, and the frames as they come as MJPEG, for a manager with a ``jpeg.JpegEncoder`` - and the faces of that frame
with their thumbnails, for a manager with ``chips.FaceChips``."""
import base64
from threading import Thread


def create_app(embedding_manager, camera_manager):
    from flask import Flask, Response, jsonify, request
    app = Flask(__name__)

    @app.after_request
    def _cors(resp):                          # flask_cors.CORS(app) equivalent (infrenceServer.py:34)
        resp.headers["Access-Control-Allow-Origin"] = "*"
        resp.headers["Access-Control-Allow-Headers"] = "Content-Type"
        return resp

    @app.route("/api/embeddings/stats", methods=["GET"])
    def get_embedding_stats():
        return jsonify(embedding_manager.get_stats())

    @app.route("/api/embeddings/sync", methods=["POST"])
    def force_sync():
        try:
            embedding_manager.force_sync()
            return jsonify({"status": "success", "message": "Sync completed"})
        except Exception as e:
            return jsonify({"status": "error", "message": str(e)}), 500

    @app.route("/api/camera/start", methods=["POST"])
    def start_camera():
        data = request.json
        sources = data.get("sources", [0])
        company_id = data.get("company_id")
        if not company_id:
            return jsonify({"status": "error", "message": "Company ID required"}), 400
        try:
            Thread(target=camera_manager.start_cameras, args=(sources, company_id), daemon=True).start()
            return jsonify({"status": "success", "message": "Camera started"})
        except Exception as e:
            return jsonify({"status": "error", "message": str(e)}), 500

    @app.route("/api/camera/stop", methods=["POST"])
    def stop_camera():
        try:
            camera_manager.stop_cameras()
            return jsonify({"status": "success", "message": "Camera stopped"})
        except Exception as e:
            return jsonify({"status": "error", "message": str(e)}), 500

    def _jpeg_source():
        """(source, None), or (None, the 404 answer): the manager must encode and know the source the query names"""
        if getattr(camera_manager, "encode", None) is None:
            return None, (jsonify({"status": "error", "message": "The camera manager has no JPEG encoder"}), 404)
        source = camera_manager.source_named(request.args.get("source", "0"))
        if source is None:
            return None, (jsonify({"status": "error", "message": "No frame from this source"}), 404)
        return source, None

    @app.route("/api/camera/snapshot", methods=["GET"])
    def camera_snapshot():
        source, refusal = _jpeg_source()
        data = None if source is None else camera_manager.latest_jpeg(source)
        if data is None:
            return refusal or (jsonify({"status": "error", "message": "No frame from this source"}), 404)
        return Response(data, mimetype="image/jpeg", headers={"Cache-Control": "no-store"})

    @app.route("/api/camera/stream", methods=["GET"])
    def camera_stream():
        source, refusal = _jpeg_source()
        if source is None:
            return refusal

        def parts():                              # one part per new frame; ends when the cameras have stopped
            count = 0
            while True:
                count, data = camera_manager.latest_jpeg(source, after=count, timeout=1.0)
                if data is None:
                    if not getattr(camera_manager, "running", False):
                        return
                    continue
                yield (b"--frame\r\nContent-Type: image/jpeg\r\nContent-Length: " + str(len(data)).encode() + b"\r\n\r\n"
                       + data + b"\r\n")
        return Response(parts(), mimetype="multipart/x-mixed-replace; boundary=frame", headers={"Cache-Control": "no-store"})

    def camera_faces():
        """the faces of the source's last processed frame: a list of {bbox, person_info, recognition_score, detection_score,
        chip}, chip the thumbnail's JPEG in base64 or null"""
        source = camera_manager.source_named(request.args.get("source", "0"))
        faces = None if source is None else camera_manager.latest_faces(source)
        if faces is None:
            return jsonify({"status": "error", "message": "No faces from this source"}), 404
        out = []
        for r in faces:
            chip = r.get("chip")
            out.append({"bbox": [int(v) for v in r["bbox"]], "person_info": r.get("person_info"),
                        "recognition_score": float(r.get("recognition_score") or 0), "detection_score": float(r.get("det_score") or 0),
                        "chip": base64.b64encode(chip).decode("ascii") if isinstance(chip, (bytes, bytearray)) else None})
        return jsonify(out)

    if hasattr(camera_manager, "latest_faces"):   # a manager that keeps faces (CameraManager): one that does not has no such route
        app.add_url_rule("/api/camera/faces", view_func=camera_faces, methods=["GET"])

    return app
