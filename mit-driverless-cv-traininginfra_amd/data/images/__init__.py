"""Real-image detector batches: `ImageLabelBatches` stands where `DataLoader(ImageLabelDataset(...))` stands in CVC-YOLOv3/train.py:124-141.

The host decodes (Pillow, on a thread pool) and crops each frame to the source window its output patch reads; everything from that
uint8 window to the `[B,C,H,W]` fp32 batch runs on the device (batch.py has the launches).  What the reference's chain computes
(CVC-YOLOv3/utils/datasets.py:124-315 with utils/utils.py's geometry and label helpers, torchvision 0.3's pad / resize / to_grayscale /
hflip / to_tensor over Pillow) is reproduced exactly; each module states its part of that contract: resample.py the images, geometry.py
the frame layout, labels.py the labels, augment.py the augmentation, the imgaug options and the random draws, loader.py the options.
"""
from ... import _lib  # noqa: F401
from ..staging import align as _align  # noqa: F401
from .augment import (AUG_DESC, BRIGHTNESS, CONTRAST, FX_DESC, FX_MAX_R, HUE, SATURATION, Augmentation, ImageFx,  # noqa: F401
                      aug_descriptor, blur_radius, blur_table, draw_augmentation, draw_imgfx, fx_descriptor, hue_shift,
                      inverse_affine_matrix, sharpen_coefficients, sigmoid_table)
from .batch import DESC, FREF, STAGED, Layout, launch_batch, pack_batch, pack_layout, transform_batch  # noqa: F401
from .geometry import (Geometry, crop_window, frame_reference, letterbox, n_patches, patch_box, sample_geometry,  # noqa: F401
                       scaled_size, tile_grid)
from .labels import affine_labels, filter_and_offset_labels, read_label_csv, sample_labels  # noqa: F401
from .loader import ImageLabelBatches  # noqa: F401
from .resample import BILINEAR, LANCZOS, PRECISION_BITS, resample_coeffs  # noqa: F401

UNSUPPORTED = ()                         # every option of the reference's ImageLabelDataset is implemented
