"""ctypes binding of libmdcv_hip.so, of libmdcv_aug.so and libmdcv_kptaug.so (device work outside the training step: `aug_lib()`,
DESIGN §29; `kptaug_lib()`), of libmdcv_cls.so (the opt-in class loss of the YOLO head: `cls_lib()`), of
libmdcv_box.so (its opt-in box loss: `box_lib()`), of libmdcv_ign.so (the opt-in prediction-IoU ignore rule of its
no-object term: `ign_lib()`), of libmdcv_mcdet.so (the opt-in class-aware detection post-processing: `mcdet_lib()`,
DESIGN §34), of libmdcv_mctiles.so (the opt-in class-aware cross-tile merge: `mctiles_lib()`), of libmdcv_softnms.so
(the opt-in Soft-NMS post-processing: `softnms_lib()`), of libmdcv_softtiles.so (the opt-in soft cross-tile merge:
`softtiles_lib()`), of libmdcv_pnp.so (the opt-in cone pose solver: `pnp_lib()`) and of libmdcv_track.so (the
opt-in tracker: `track_lib()`).

Prototypes are parsed from ``include/mdcv_hip.h`` (``include/mdcv_aug.h``) so the header is the single source of truth for the C ABI.
There is NO CPU fallback: if the shared library is missing, or an entry point is asked to run without a GPU, this
module fails loudly (the oracle under ``oracle/`` is test infrastructure and is never imported from here).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(ROOT, "include", "mdcv_hip.h")
LIB_PATH = os.environ.get("MDCV_LIB") or os.path.join(_HERE, "libmdcv_hip.so")      # MDCV_LIB: another BUILD of the same library (timing ablations, scripts/wgrad_ab.py)

AUG_HEADER = os.path.join(ROOT, "include", "mdcv_aug.h")
AUG_LIB_PATH = os.path.join(_HERE, "libmdcv_aug.so")

KPTAUG_HEADER = os.path.join(ROOT, "include", "mdcv_kptaug.h")
KPTAUG_LIB_PATH = os.path.join(_HERE, "libmdcv_kptaug.so")

CLS_HEADER = os.path.join(ROOT, "include", "mdcv_cls.h")
CLS_LIB_PATH = os.path.join(_HERE, "libmdcv_cls.so")
CLS_MODES = {"ce": 0, "bce": 1}                  # include/mdcv_cls.h MDCV_CLS_CE / MDCV_CLS_BCE
CLS_ERR_WORD = 3                                 # int32 index of the err word in a class workspace (MDCV_CLS_ERR_WORD)

BOX_HEADER = os.path.join(ROOT, "include", "mdcv_box.h")
BOX_LIB_PATH = os.path.join(_HERE, "libmdcv_box.so")
BOX_MODES = {"giou": 0, "diou": 1, "ciou": 2}    # include/mdcv_box.h MDCV_BOX_GIOU / MDCV_BOX_DIOU / MDCV_BOX_CIOU

IGN_HEADER = os.path.join(ROOT, "include", "mdcv_ign.h")
IGN_LIB_PATH = os.path.join(_HERE, "libmdcv_ign.so")

MCDET_HEADER = os.path.join(ROOT, "include", "mdcv_mcdet.h")
MCDET_LIB_PATH = os.path.join(_HERE, "libmdcv_mcdet.so")
MCDET_MAX_CLASSES = 65535                        # include/mdcv_mcdet.h MDCV_MCDET_MAX_CLASSES

MCTILES_HEADER = os.path.join(ROOT, "include", "mdcv_mctiles.h")
MCTILES_LIB_PATH = os.path.join(_HERE, "libmdcv_mctiles.so")
# the cross-tile merge of the tiled detectors: mdcv_detect_merge_tiles / _mc, and mdcv_detect_merge_tiles_soft without / with classes
TILE_MERGES = ("agnostic", "per_class", "soft", "soft_per_class")
SOFT_TILE_MERGES = ("soft", "soft_per_class")

SOFTNMS_HEADER = os.path.join(ROOT, "include", "mdcv_softnms.h")
SOFTNMS_LIB_PATH = os.path.join(_HERE, "libmdcv_softnms.so")
SOFTTILES_HEADER = os.path.join(ROOT, "include", "mdcv_softtiles.h")
SOFTTILES_LIB_PATH = os.path.join(_HERE, "libmdcv_softtiles.so")
PNP_HEADER = os.path.join(ROOT, "include", "mdcv_pnp.h")
PNP_LIB_PATH = os.path.join(_HERE, "libmdcv_pnp.so")
TRACK_HEADER = os.path.join(ROOT, "include", "mdcv_track.h")
TRACK_LIB_PATH = os.path.join(_HERE, "libmdcv_track.so")
NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}   # include/mdcv_softnms.h MDCV_SNMS_HARD / _LINEAR / _GAUSSIAN

F32, BF16 = 0, 1


def tuned(dtype, code):
    """dtype argument carrying a per-call variant code (include/mdcv_hip.h MDCV_TUNED; csrc/tune.h lists the codes; 0 = defaults)"""
    return (dtype & 0xff) | (int(code) * 256)
ACT_NONE, ACT_LEAKY, ACT_RELU = 0, 1, 2

_CT = {
    "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
}


def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p            # every pointer crosses as an address (torch .data_ptr() / int / None)
    decl = re.sub(r"\b(const|unsigned)\b", "", decl).strip()
    base = " ".join(decl.split()[:-1]) if len(decl.split()) > 1 else decl
    return _CT[base]


def parse_header(path=HEADER):
    """-> {name: (restype, [argtypes], [argnames])} for every ``mdcv_*`` prototype in the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int|long long)\s+(mdcv_\w+)\s*\(([^)]*)\)\s*;", text):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        argl = [a for a in (x.strip() for x in args.split(",")) if a and a != "void"]
        names = [re.split(r"[\s\*]+", a)[-1] for a in argl]
        protos[name] = (_CT[ret], [_ctype(a) for a in argl], names)
    return protos


class MdcvError(RuntimeError):
    pass


class _Lib:
    def __init__(self, path=None, header=None, name="libmdcv_hip"):
        path, header, self.name = path or LIB_PATH, header or HEADER, name
        if not os.path.exists(path):
            raise MdcvError(
                f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C {os.path.join(_HERE, 'csrc')}`). There is no CPU fallback for the product path.")
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).  It must be in the process
        # BEFORE our library is dlopen'ed so that both bind to the same runtime instance; two runtimes in one process
        # do not share devices/streams (kernels launched through the second one fail with hipErrorNoDevice).
        import torch  # noqa: F401
        self.cdll = ctypes.CDLL(path)
        self.protos = parse_header(header)
        for name, (ret, argt, _) in self.protos.items():
            fn = getattr(self.cdll, name)       # AttributeError here == header/library mismatch
            fn.restype = ret
            fn.argtypes = argt
            setattr(self, name[len("mdcv_"):], fn)

    def check(self, rc, what=""):
        if rc != 0:
            raise MdcvError(f"{self.name}: {what} failed with code {rc}" + (" (bad argument)" if rc == -1 else " (hipError_t)"))


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib


_aug = None


def aug_lib():
    """libmdcv_aug.so behind include/mdcv_aug.h: the same binding and the same `check` as `lib()`, loaded on first use"""
    global _aug
    if _aug is None:
        _aug = _Lib(AUG_LIB_PATH, AUG_HEADER, "libmdcv_aug")
    return _aug


_kptaug = None


def kptaug_lib():
    """libmdcv_kptaug.so behind include/mdcv_kptaug.h: the same binding and `check` again, loaded on first use"""
    global _kptaug
    if _kptaug is None:
        _kptaug = _Lib(KPTAUG_LIB_PATH, KPTAUG_HEADER, "libmdcv_kptaug")
    return _kptaug


_cls = None


def cls_lib():
    """libmdcv_cls.so behind include/mdcv_cls.h: the same binding and `check`, loaded on first use -- by a model built
    with cls_loss != 0 only"""
    global _cls
    if _cls is None:
        _cls = _Lib(CLS_LIB_PATH, CLS_HEADER, "libmdcv_cls")
    return _cls


def cls_mode(name):
    if name not in CLS_MODES:
        raise ValueError(f"cls_mode must be one of {sorted(CLS_MODES)}, got {name!r}")
    return CLS_MODES[name]


_box = None


def box_lib():
    """libmdcv_box.so behind include/mdcv_box.h: the same binding and `check`, loaded on first use -- by a model built
    with box_loss != 0 only"""
    global _box
    if _box is None:
        _box = _Lib(BOX_LIB_PATH, BOX_HEADER, "libmdcv_box")
    return _box


def box_mode(name):
    if name not in BOX_MODES:
        raise ValueError(f"box_mode must be one of {sorted(BOX_MODES)}, got {name!r}")
    return BOX_MODES[name]


_ign = None


def ign_lib():
    """libmdcv_ign.so behind include/mdcv_ign.h: the same binding and `check`, loaded on first use -- by a model built
    with pred_ignore != 0 only"""
    global _ign
    if _ign is None:
        _ign = _Lib(IGN_LIB_PATH, IGN_HEADER, "libmdcv_ign")
    return _ign


_mcdet = None


def mcdet_lib():
    """libmdcv_mcdet.so behind include/mdcv_mcdet.h: the same binding and `check`, loaded on first use -- by a
    class_aware=True post-processing call or an nms(..., classes=) only"""
    global _mcdet
    if _mcdet is None:
        _mcdet = _Lib(MCDET_LIB_PATH, MCDET_HEADER, "libmdcv_mcdet")
    return _mcdet


_mctiles = None


def mctiles_lib():
    """libmdcv_mctiles.so behind include/mdcv_mctiles.h: the same binding and `check`, loaded on first use -- by a tiled
    detector built with class_aware=True, tile_merge="per_class" only"""
    global _mctiles
    if _mctiles is None:
        _mctiles = _Lib(MCTILES_LIB_PATH, MCTILES_HEADER, "libmdcv_mctiles")
    return _mctiles


_softnms = None


def softnms_lib():
    """libmdcv_softnms.so behind include/mdcv_softnms.h: the same binding and `check`, loaded on first use -- by a
    post-processing call or an nms() with a soft method, or by soft_nms(), only"""
    global _softnms
    if _softnms is None:
        _softnms = _Lib(SOFTNMS_LIB_PATH, SOFTNMS_HEADER, "libmdcv_softnms")
    return _softnms


_softtiles = None


def softtiles_lib():
    """libmdcv_softtiles.so behind include/mdcv_softtiles.h: the same binding and `check`, loaded on first use -- by a tiled
    detector built with tile_merge="soft" / "soft_per_class" only"""
    global _softtiles
    if _softtiles is None:
        _softtiles = _Lib(SOFTTILES_LIB_PATH, SOFTTILES_HEADER, "libmdcv_softtiles")
    return _softtiles


_pnp = None


def pnp_lib():
    """libmdcv_pnp.so behind include/mdcv_pnp.h: the same binding and `check`, loaded on first use -- by
    mdcv.rektnet.pose.solve_cone_pnp only"""
    global _pnp
    if _pnp is None:
        _pnp = _Lib(PNP_LIB_PATH, PNP_HEADER, "libmdcv_pnp")
    return _pnp


_track = None


def track_lib():
    """libmdcv_track.so behind include/mdcv_track.h: the same binding and `check`, loaded on first use -- by
    mdcv.yolo.track.track_boxes and a detector's first batch with `track=` only"""
    global _track
    if _track is None:
        _track = _Lib(TRACK_LIB_PATH, TRACK_HEADER, "libmdcv_track")
    return _track


def nms_method(who, name, sigma=0.5):
    """the method's code; an unknown name, or a sigma that is not a positive finite number with "gaussian", is a ValueError"""
    if name not in NMS_METHODS:
        raise ValueError(f"{who}: nms method must be one of {sorted(NMS_METHODS)}, got {name!r}")
    if name == "gaussian" and not 0.0 < float(sigma) < float("inf"):
        raise ValueError(f"{who}: sigma must be a positive finite number with the gaussian nms method, got {sigma!r}")
    return NMS_METHODS[name]


def pred_ignore(value):
    """the threshold as a float: 0 is off, anything outside [0, 1) a ValueError (NaN included)"""
    v = float(value)
    if not 0.0 <= v < 1.0:
        raise ValueError(f"pred_ignore must lie in [0, 1) (0 = off), got {value!r}")
    return v


def require_gpu(t=None):
    import torch
    if not torch.cuda.is_available():
        raise MdcvError("MDCV HIP path needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    if t is not None and not t.is_cuda:
        raise MdcvError("MDCV HIP path got a CPU tensor: move the model and inputs to the GPU (`.to('cuda')`)")
