"""Drop-in for the reference's RektNet hot-path modules (keypoint_net.py, resnet.py, cross_ratio_loss.py), and the batched form of
train_eval.py's two validation routines (evaluate.py) and the native form of its training loop (train.py)."""
from .evaluate import KeypointEvaluator, eval_model, print_kpt_L2_distance  # noqa: F401
from .train import train_model  # noqa: F401
