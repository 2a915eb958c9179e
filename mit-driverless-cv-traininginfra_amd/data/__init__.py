"""Detector and key-point batches on the GPU: synthetic cones, and real images and real cone crops with the reference's dataset contracts; and the
stage in front of them, dataset preparation (camera scales, k-means anchors on the device, the CSV splits); and mosaic augmentation of a
finished detector batch (four images of the batch composed into each); and affine, flip and colour augmentation of a finished key-point batch
(DESIGN §30)."""
from .synth import SyntheticCones, SyntheticConeCrops  # noqa: F401
from .images import ImageLabelBatches  # noqa: F401
from .crops import ConeCropBatches, load_train_csv_dataset  # noqa: F401
from .prep import kmeans_anchors, prepare_dataset  # noqa: F401
from .mosaic import MosaicBatches  # noqa: F401
from .kptaug import KeypointAugBatches  # noqa: F401
