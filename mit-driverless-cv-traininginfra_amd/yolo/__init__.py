"""Drop-in for the reference's CVC-YOLOv3 hot-path modules (models.py, utils/utils.py, utils/parse_config.py)."""


def __getattr__(name):
    # the dataset-level evaluator's names (mdcv/yolo/evaluate.py), resolved on first use: importing the package stays as cheap as it was
    # (`mdcv.yolo.evaluate` itself is the module, as `mdcv.yolo.validate` is: its function is `mdcv.yolo.evaluate.evaluate`)
    if name in ("DatasetAP", "APResult", "evaluate_frames", "COCO_IOU_THRESHOLDS"):
        import importlib
        return getattr(importlib.import_module(__name__ + ".evaluate"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
