"""Detector and key-point batches on the GPU: synthetic cones, and real images with the reference's dataset contract."""
from .synth import SyntheticCones, SyntheticConeCrops  # noqa: F401
from .images import ImageLabelBatches  # noqa: F401
