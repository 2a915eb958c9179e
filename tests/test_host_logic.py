"""CPU-only tests of the host side: cfg parser, module construction / state_dict / .weights I/O (no compute), the C-ABI
library's exports, the no-CPU-fallback rule, the oracle-isolation rule."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "mit-driverless-cv-traininginfra_amd")


def test_library_exports_every_declared_symbol():
    from mdcv import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 40
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (mdcv_\w+)", out))
    assert exported == set(protos), exported ^ set(protos)       # header and library agree exactly


def test_argument_errors_are_reported_without_a_gpu():
    from mdcv import _lib
    L = _lib.lib()
    assert L.conv2d(1, 0, None, 8, None, None, 8, None, None, 0, None, 1, 4, 4, 8, 4, 4, 8, 3, 3, 1, 1, 1, None) == -1
    assert L.conv2d_stats_rows(129) == 2
    assert L.conv2d_wgrad_splits(1, 100000, 256, 1152) >= 1
    assert L.yolo_head_workspace_bytes(2, 3, 13, 13) > 0


def test_stride2_weight_gradients_dispatch_to_the_parity_plane_kernel():
    """Host side of mdcv_conv2d_wgrad's dispatch (no GPU): Darknet-53's five down-sampling layers (reference yolo_baseline.cfg, the `stride=2`
    [convolutional] blocks at batch 32) size their slab workspace by the parity-plane ring kernel's split rule (csrc/wgrad_stream_s2.hip: 256
    blocks of 64 co x 32 ci tiles), variant 34060 by the generic kernel's; odd inputs and channel counts the ring kernel does not tile stay generic."""
    from mdcv import _lib
    L = _lib.lib()
    for Ho, Ci, Co, want in ((13, 512, 1024, 1), (26, 256, 512, 4), (52, 128, 256, 16), (104, 64, 128, 64), (208, 32, 64, 254)):
        H = 2 * Ho
        tiles = (Co // 64) * (Ci // 32)
        assert L.conv2d_wgrad_splits_geom(1, 32, H, H, Ci, Ho, Ho, Co, 3, 3, 2, 1, 1, Co, Ci) == want
        assert 192 <= want * tiles <= 256
    generic = L.conv2d_wgrad_splits_geom(_lib.tuned(1, 34060), 32, 104, 104, 128, 52, 52, 256, 3, 3, 2, 1, 1, 256, 128)
    assert generic != 16
    assert L.conv2d_wgrad_splits_geom(1, 32, 105, 105, 128, 53, 53, 256, 3, 3, 2, 1, 1, 256, 128) == \
        L.conv2d_wgrad_splits_geom(_lib.tuned(1, 34060), 32, 105, 105, 128, 53, 53, 256, 3, 3, 2, 1, 1, 256, 128)          # odd input
    assert L.conv2d_wgrad_splits_geom(1, 32, 104, 104, 48, 52, 52, 256, 3, 3, 2, 1, 1, 256, 48) == \
        L.conv2d_wgrad_splits_geom(_lib.tuned(1, 34060), 32, 104, 104, 48, 52, 52, 256, 3, 3, 2, 1, 1, 256, 48)            # Cin % 32 != 0


def test_product_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mdcv import _lib
    from mdcv.rektnet.keypoint_net import KeypointNet
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    with pytest.raises(_lib.MdcvError):
        KeypointNet()(torch.zeros(1, 3, 80, 80))
    with pytest.raises(_lib.MdcvError):
        CrossRatioLoss("l1_softargmax", True, 0.0, 0.0)(None, torch.zeros(2, 7, 2), None, torch.zeros(2, 7, 2))
    cwd = os.getcwd()
    os.chdir(os.path.join(G, "mini"))
    try:
        from mdcv.yolo.models import Darknet
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
    finally:
        os.chdir(cwd)
    with pytest.raises(_lib.MdcvError):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 1, 5))


def test_product_never_imports_oracle():
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|/oracle/|oracle\.", re.M)
    for dp, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                code = "\n".join(l for l in txt.split("\n") if not l.strip().startswith(("#", "//", "*", '"""')))
                assert not pat.search(code), os.path.join(dp, f)


def test_parse_model_config_contract(tmp_path):
    from mdcv.yolo.utils.parse_config import parse_model_config
    p = tmp_path / "a.cfg"
    p.write_text("# comment\n[net]\n width = 64 \nheight=64\n\n[convolutional]\nfilters=16\nsize=3\nstride=1\n  [route]\nlayers = -1, 4\n")
    d = parse_model_config(str(p))
    assert d[0] == {"type": "net", "width": "64", "height": "64"}
    assert d[1] == {"type": "convolutional", "batch_normalize": 0, "filters": "16", "size": "3", "stride": "1"}
    assert d[2] == {"type": "route", "layers": "-1, 4"}
    from oracle.yolo_oracle import parse_cfg
    assert parse_cfg(os.path.join(G, "mini", "mini.cfg")) == parse_model_config(os.path.join(G, "mini", "mini.cfg"))


def test_darknet_structure_state_dict_and_weights_io(tmp_path):
    z = np.load(os.path.join(G, "mini_darknet.npz"))
    cwd = os.getcwd()
    os.chdir(os.path.join(G, "mini"))
    try:
        from mdcv.yolo.models import Darknet, YOLOLayer
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    assert list(net.state_dict().keys()) == [str(k) for k in z["param_names"]]
    assert net.get_anchors() == [[4.0, 6.0], [6.0, 10.0], [10.0, 8.0], [12.0, 20.0], [20.0, 16.0], [24.0, 36.0]]
    assert net.get_loss_constant() == [2.0, 1.6, 25.0, 0.1] and net.img_size() == (64, 64) and net.get_threshs() == (0.8, 0.25, 0.5)
    assert net.get_onnx_name() == "mini_6464.onnx" and net.get_num_classes() == 1 and net.get_bw() is False
    yl = [m[0] for m in net.module_list if isinstance(m[0], YOLOLayer)]
    assert yl[0].anchors == [[12.0, 20.0], [20.0, 16.0], [24.0, 36.0]] and yl[1].anchors == [[4.0, 6.0], [6.0, 10.0], [10.0, 8.0]]
    p = tmp_path / "rt.weights"
    net.save_weights(str(p))
    assert open(p, "rb").read() == open(os.path.join(G, "mini", "mini.weights"), "rb").read()
    # an 80-class file initialises a narrower head through start_weight_dim (Q13): emulate with 18 -> keep first 12 filters
    from oracle.yolo_oracle import DarknetOracle, read_anchor_row
    os.chdir(os.path.join(G, "mini"))
    try:
        orc = DarknetOracle("mini.cfg", anchors=read_anchor_row("dataset/train.csv"))
        orc.load_weights("mini.weights", [18, 18])
    finally:
        os.chdir(cwd)
    sd = net.state_dict()
    assert torch.equal(sd["module_list.11.conv_11.weight"], orc.params["conv11.weight"])
    assert torch.equal(sd["module_list.3.batch_norm_3.running_var"], orc.params["bn3.running_var"])


def test_keypointnet_state_dict_matches_reference_names():
    from mdcv.rektnet.keypoint_net import KeypointNet
    z = np.load(os.path.join(G, "rektnet_net.npz"))
    torch.manual_seed(0)
    net = KeypointNet()
    ref_keys = [k[4:] for k in z.files if k.startswith("sd::")]
    assert list(net.state_dict().keys()) == ref_keys
    assert sum(p.numel() for p in net.parameters()) == 311383
    # kaiming-normal fan_out init: std = sqrt(2 / (Cout*k*k)), zero biases, BN 1/0
    w = net.res3.conv2.weight
    assert abs(float(w.std()) - (2.0 / (64 * 9)) ** 0.5) < 0.003 and float(net.conv.bias.abs().max()) == 0.0
    assert float(net.bn.weight.min()) == 1.0


def test_cross_ratio_prints_and_unknown_type():
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    crit = CrossRatioLoss("bogus", True, 0.1, 0.2)
    with pytest.raises(NameError):
        crit(None, torch.zeros(1, 7, 2), None, torch.zeros(1, 7, 2))


def test_models_with_cached_plans_deepcopy_and_pickle():
    """RektNet/train_eval.py:99 keeps `best_model = copy.deepcopy(model)` after a forward; the launch plans a forward leaves behind
    hold ctypes function pointers and closures, which must not travel with the copy (it rebuilds them lazily)."""
    import copy
    import pickle
    from mdcv.rektnet.keypoint_net import KeypointNet
    from mdcv.yolo.models import Darknet

    class FakePlan:                        # what a cached plan looks like to pickle: ctypes pointers + closures
        def __init__(self):
            self.fn = ctypes.CFUNCTYPE(ctypes.c_int)(lambda: 0)
            self.closure = lambda s: 0

    cwd = os.getcwd()
    os.chdir(os.path.join(G, "mini"))
    try:
        yolo = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
    finally:
        os.chdir(cwd)
    for net in (KeypointNet(), yolo):
        net._flatten()                     # parameters become views of one flat buffer, as after the first forward
        net._plans[("k",)] = FakePlan()
        net._last_train_plan = FakePlan()
        before = {k: v.clone() for k, v in net.state_dict().items()}
        for dup in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
            assert dup._plans == {} and not hasattr(dup, "_last_train_plan") and not dup._flat_ok()
            for k, v in dup.state_dict().items():
                assert torch.equal(v, before[k]), k
            p0 = next(dup.parameters())
            with torch.no_grad():
                p0.add_(1.0)                # the copy owns its storage
            assert torch.equal(net.state_dict()[next(iter(before))], before[next(iter(before))])
        assert ("k",) in net._plans        # the original keeps its plans


def test_cross_ratio_rejects_other_keypoint_counts():
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    crit = CrossRatioLoss("l1_softargmax", True, 0.1, 0.2)
    with pytest.raises(ValueError):
        crit(None, torch.zeros(2, 5, 2), None, torch.zeros(2, 5, 2))


def test_bench_cli_contract_without_gpu():
    """bench.py refuses to run without a GPU (no CPU fallback) -- and says so instead of crashing."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode != 0 and "no CPU fallback" in (out.stderr + out.stdout)


def test_kernel_fingerprint_tracks_sources(tmp_path):
    from mdcv import _fingerprint as F
    a = F.kernel_fingerprint()
    assert a == F.kernel_fingerprint() and len(a) == 16
    assert any(f.endswith("conv_igemm.hip") for f in F.fingerprint_files()) and any(f.endswith("engine.py") for f in F.fingerprint_files())


def test_bench_line_fits_the_drivers_capture():
    """BENCH_r02.parsed was null: the final JSON line had grown to 27 KB (per-kernel tables) and the driver keeps an 8.4 KB tail.  The
    line is now assembled by build_line/compact (tables go to bench_detail.json): a full line with every optional block stays < 3.5 KB."""
    import argparse
    import json
    sys.path.insert(0, ROOT)
    import bench
    a = argparse.Namespace(steps=30, warmup=10, precision="bf16", yolo_classes=80, yolo_batch=32, rekt_batch=256, post_batch=32,
                           joint_batch=32, graph=0, workload="both")
    roof = {"kernel": "wgrad3x3_stream_kernel<4, 4, 4, 1, 64, 1, 1, true, 4>" + "x" * 120, "bound": "mfma", "launches": 31, "avg_us": 117.99512345,
            "achieved": 432.512345, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.17300012345, "timing": "in-step (live HIP event pairs, both streams running)",
            "avg_us_alone": 74.123456, "frac_alone": 0.2761234, "flops_per_launch": 51039436800.0, "traffic": 75512345.0,
            "traffic_source": "r03_pmc_hbm_traffic.json", "total_ms": 3.66, "junk": "z" * 5000}
    extra = {"yolo": {"images_per_sec": 2279.123456, "ms_per_step": 14.0412345, "global_batch": 32, "final_loss": 4.0123456, "mfma_frac_step": 0.18012345,
                      "images_per_sec_with_h2d_copy": None, "fp32_images_per_sec": 404.123456, "fp32_note": "n" * 150, "sum_kernel_ms_serial": 19.123,
                      "kernel_launches_per_step": 780, "hbm_bytes_per_step": 45163199360.0, "replicas_in_sync": True,
                      "comm": {"allreduce_busy_ms": 1.234567, "exposed_comm_ms": 0.123456, "ranks": 8, "gradient_bytes": 247796596, "bucket_mb": 32.0,
                               "backend": "rccl", "note": "n" * 200}},
             "rektnet": {"images_per_sec": 32612.123456, "ms_per_step": 7.8512345, "global_batch": 256, "final_loss": 0.1234567, "mfma_frac_step": 0.15512345,
                         "hbm_frac_step": 0.2351234, "cpu_images_per_sec": 135.12345,
                         "dominant_kernel": {"kernel": "wgrad3x3_stream_kernel<4, 8, 4, 1, 64, 2, 1, true, 8>", "bound": "mfma", "avg_us": 1264.1, "frac": 0.153, "frac_alone": 0.23}},
             "postprocess": {"images_per_sec": 527000.123, "ms_per_batch": 0.0607, "batch_per_gpu": 32, "rows_per_image": 10647, "classes": 80,
                             "kept_mean": 136.2, "mean_ap": 0.91234, "hbm_floor_us": 2.7, "cpu_images_per_sec": 659.1}}
    cb = {"value": 5.26123, "unit": "images/sec", "cores": 16, "host_cores": 256, "kind": "port", "sample": "YOLOv3 416^2 classes=80 fp32 CPU oracle, batch 4, 2 timed train steps after 1 warm-up (Adam)"}
    line = bench.build_line(a, 8, "yolo", {"value": 2279.123456789, "ms_per_step": 14.04123456789, "roofline": roof}, extra, cb)
    line["detail"] = "gpurun_out/bench_detail.json"
    out = bench.compact(line)
    txt = json.dumps(out)
    assert len(txt) <= bench.MAX_LINE_BYTES, len(txt)
    back = json.loads(txt)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "host_cores", "fingerprint"):
        assert k in back, k
    assert back["value"] == 2279.123456789 and back["ms_per_step"] == 14.04123456789        # the driver's consistency check sees full precision
    assert "junk" not in back["roofline"] and {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(back["roofline"])
    assert {"value", "unit", "cores", "kind", "sample"} <= set(back["cpu_baseline"])
    # a line that would still be too long loses its optional blocks, never the contract keys
    extra["yolo"]["blob"] = "q" * 6000
    out = bench.compact(bench.build_line(a, 1, "yolo", {"value": 1.0, "ms_per_step": 1.0, "roofline": roof}, extra, cb))
    assert "workloads" not in out and out["roofline"] and out["cpu_baseline"] and len(json.dumps(out)) <= bench.MAX_LINE_BYTES


def test_bench_dump_outputs_samples_large_outputs_the_same_way(tmp_path):
    """bench.py --dump-outputs: small outputs keep their shape, a large one is a seeded sample of fixed positions, integer indices come out
    float64 and everything else float32, and more than 64 MB in all is refused."""
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32)
    arrays = {"loss": torch.tensor([1.5, 2.5]), "big": big, "idx": torch.arange(5), "h": torch.ones(2, 3, dtype=torch.bfloat16)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in arrays}
    assert a["loss"].dtype == np.float32 and a["loss"].tolist() == [1.5, 2.5]
    assert a["idx"].dtype == np.float64 and a["h"].dtype == np.float32 and a["h"].shape == (2, 3)
    assert a["big"].ndim == 1 and bench.DUMP_SAMPLE // 2 < a["big"].size <= bench.DUMP_SAMPLE
    assert np.all(np.diff(a["big"]) > 0) and np.array_equal(a["big"], b["big"])       # sorted positions, the same in both runs
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), {f"t{i}": big for i in range(12)})


_SHIM_PROBE = r"""
import importlib.util, os, sys
shim, ref = sys.argv[1], sys.argv[2]
sys.path[:0] = [shim, ref]                      # the shim directory in front of the reference's script directory
os.chdir(ref)
if os.path.basename(shim) == "CVC-YOLOv3":
    from models import Darknet, YOLOLayer, create_modules, EmptyLayer, vanilla_anchor_list, parse_model_config     # train.py:19, validate.py:12
    import models
    assert Darknet.__module__.startswith("mdcv.yolo.models"), Darknet.__module__
    for name in ("utils", "utils.nms", "utils.utils", "utils.datasets", "validate"):
        spec = importlib.util.find_spec(name)
        assert spec is not None and os.path.realpath(spec.origin).startswith(os.path.realpath(ref)), (name, spec)
    if os.environ.get("SHIM_FAKE_TREE"):
        from utils.utils import model_info, Logger                      # train.py:21 -> the reference tree's helpers
        import validate                                                 # train.py:22 -> its validate.py, which did `from utils.nms import nms`
        assert model_info() == "reference-tree helper" and validate.nms() == "reference nms"
        assert sorted(models.use_hip_postprocessing()) == ["utils.nms.nms", "validate.nms"]
        import utils.nms
        assert utils.nms.nms.__module__ == "mdcv.yolo.utils.nms" and validate.nms is utils.nms.nms
else:
    from keypoint_net import KeypointNet                                # train_eval.py:24
    from cross_ratio_loss import CrossRatioLoss                         # train_eval.py:25
    from resnet import ResNet
    assert KeypointNet.__module__ == "mdcv.rektnet.keypoint_net" and CrossRatioLoss.__module__ == "mdcv.rektnet.cross_ratio_loss"
    for name in ("utils", "dataset"):                                   # train_eval.py:26-28 -> the reference's own RektNet/utils.py, dataset.py
        spec = importlib.util.find_spec(name)
        assert spec is not None and os.path.realpath(spec.origin).startswith(os.path.realpath(ref)), (name, spec)
    assert sum(p.numel() for p in KeypointNet().parameters()) == 311383
print("SHIM_OK")
"""


def _fake_reference_tree(tmp_path):
    """A stand-in with the reference's script-directory layout (module NAMES only; the bodies are test stubs)."""
    y = tmp_path / "CVC-YOLOv3"
    (y / "utils").mkdir(parents=True)
    (y / "utils" / "__init__.py").write_text("")
    (y / "utils" / "nms.py").write_text("def nms(*a, **k):\n    return 'reference nms'\n")
    (y / "utils" / "utils.py").write_text("def model_info(*a):\n    return 'reference-tree helper'\n\n\nclass Logger:\n    pass\n")
    (y / "utils" / "datasets.py").write_text("class ImageLabelDataset:\n    pass\n")
    (y / "validate.py").write_text("from models import Darknet\nfrom utils.nms import nms\n")
    (y / "models.py").write_text("raise ImportError('the shim must win over the reference models.py')\n")
    r = tmp_path / "RektNet"
    r.mkdir()
    (r / "utils.py").write_text("class Logger:\n    pass\n")
    (r / "dataset.py").write_text("class ConeDataset:\n    pass\n")
    for m in ("keypoint_net", "cross_ratio_loss", "resnet"):
        (r / (m + ".py")).write_text("raise ImportError('the shim must win')\n")
    return str(y), str(r)


@pytest.mark.parametrize("which", ["CVC-YOLOv3", "RektNet"])
def test_dropin_shims_import_exactly_as_the_reference_scripts_do(tmp_path, which):
    """`PYTHONPATH=<repo>/dropin/<dir> python train.py` -- `from models import Darknet` / `from keypoint_net import
    KeypointNet` / `from cross_ratio_loss import CrossRatioLoss` bind the HIP classes while `utils`, `utils.*`, `validate`, `dataset` keep
    resolving to the reference's own tree (round 2's recipe put a whole package directory on sys.path and raised ImportError)."""
    shim = os.path.join(ROOT, "dropin", which)
    assert sorted(f for f in os.listdir(shim) if not f.startswith("__")) == (["models.py"] if which == "CVC-YOLOv3" else
                                                                              ["cross_ratio_loss.py", "keypoint_net.py", "resnet.py"])
    fake_y, fake_r = _fake_reference_tree(tmp_path)
    trees = [(fake_y if which == "CVC-YOLOv3" else fake_r, "1")]
    real = os.path.join("/root/reference", which)
    if os.path.isdir(real):                         # build container only: the real layout (its helpers need PIL / cv2, so only located, not imported)
        trees.append((real, ""))
    for ref, fake in trees:
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        out = subprocess.run([sys.executable, "-c", _SHIM_PROBE, shim, ref], capture_output=True, text=True, env=dict(env, SHIM_FAKE_TREE=fake), cwd=str(tmp_path))
        assert out.returncode == 0 and "SHIM_OK" in out.stdout, (ref, out.stdout[-500:], out.stderr[-1500:])


def test_data_parallel_replication_fails_loudly():
    """reference train.py:193-195 wraps the model in nn.DataParallel when more than one GPU is visible; replicating a model that owns
    flat buffers, launch plans and side streams must raise a clear error instead of running replicas on device 0's memory."""
    from mdcv.rektnet.keypoint_net import KeypointNet
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(os.path.join(G, "mini"))
    try:
        yolo = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
    finally:
        os.chdir(cwd)
    for net in (yolo, KeypointNet()):
        with pytest.raises(RuntimeError, match="one process per GPU"):
            torch.nn.parallel.replicate(net, [0, 1]) if torch.cuda.device_count() > 1 else net._replicate_for_data_parallel()
        assert isinstance(torch.nn.DataParallel(net, device_ids=None if torch.cuda.is_available() else []).module, type(net))   # wrapping alone is fine


def test_autocast_gradient_curve_fixture_is_what_the_gpu_test_expects():
    """tests/golden/yolo_autocast_bf16_cos.json (tests/golden/make_golden.py autocast: the REFERENCE's Darknet under torch.autocast(bfloat16)
    against itself in fp32): one cosine per conv layer of yolo_baseline, at the batch / seeds the full-size GPU parity test uses; head convs
    aligned, conv 0 not."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = json.load(open(os.path.join(root, "tests", "golden", "yolo_autocast_bf16_cos.json")))
    assert os.path.exists(os.path.join(root, d["generator"].split()[0])) and "REFERENCE" in d["what"]
    assert (d["batch"], d["size"], d["oracle_seed"], d["data_seed"], d["targets_per_image"]) == (32, 416, 3, 21, 16)
    assert len(d["cos"]) == 75 and all(0.3 < v <= 1.0 for v in d["cos"].values())
    for head in ("conv81.weight", "conv93.weight", "conv105.weight"):
        assert d["cos"][head] > 0.999
    assert d["cos"]["conv0.weight"] < 0.6 and abs(d["loss"]["bf16"] / d["loss"]["fp32"] - 1) < 5e-3


def test_ring_kernels_drain_their_lds_reads_before_every_barrier():
    """ISA check of the library as built (scripts/check_ring_barriers.py): in every gfx950 kernel that refills LDS with LDS-DMA, no path
    reaches an s_barrier with ds_reads of the wave still queued.  A queued read behind the barrier races with another wave's DMA into
    the slot it reads (an LDS-DMA write is not ordered against queued ds_reads), and the compiler moves a step's last MFMAs -- with the
    s_waitcnt that guards their fragments -- below the next barrier unless the kernel pins them: round 3 found that as one wrong
    16-column fragment per ~2000 YOLOv3 steps.  Needs only the built .so and llvm-objdump (no GPU)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "mit-driverless-cv-traininginfra_amd", "libmdcv_hip.so")
    if not os.path.exists(lib):
        sys.path.insert(0, root)
        import __graft_entry__
        __graft_entry__.build()
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    sys.path.insert(0, os.path.join(root, "scripts"))
    import check_ring_barriers
    seen, bad = check_ring_barriers.check(lib)
    assert seen >= 100, seen                              # the conv / shift / weight-gradient families are all LDS-DMA kernels
    assert not bad, bad[:10]


def test_bench_comm_preflight_turns_a_failing_lease_into_a_diagnosis():
    """`bench.py --gpus N` opens with comm_preflight: when the process group cannot come up -- here: the RCCL backend on a
    box without a GPU, no rendezvous peer -- rank 0 prints ONE JSON object naming the failing step and the environment, and exits with 3 instead of
    leaving the driver with a traceback and a return code."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import torch, bench; "
            "bench.comm_preflight('nccl', 0, 2, torch.device('cpu'))" % root)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 3, (out.returncode, out.stdout[-500:], out.stderr[-1500:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["error"] == "data-parallel preflight failed" and d["step"] == "init_process_group" and d["world"] == 2 and d["backend"] == "nccl"
    assert "exception" in d and "hint" in d and "HSA_ENABLE_IPC_MODE_LEGACY" in d


def _reference_shapes(net, size):
    """(C, H, W) per section from the stock nn modules on a batch-1 zero tensor: route = torch.cat, shortcut = add (reference models.py:312-338)."""
    x = torch.zeros(1, int(net.hyperparams["channels"]), size, size)
    outs = []
    with torch.no_grad():
        for i, (d, m) in enumerate(zip(net.module_defs, net.module_list)):
            k = d["type"]
            if k in ("convolutional", "upsample", "maxpool"):
                x = m(x)
            elif k == "route":
                x = torch.cat([outs[i + int(t) if int(t) < 0 else int(t)] for t in d["layers"].split(",")], 1)
            elif k == "shortcut":
                x = outs[-1] + outs[i + int(d["from"]) if int(d["from"]) < 0 else int(d["from"])]
            outs.append(x)                                   # ([yolo] passes its input on)
    return [tuple(o.shape[1:]) for o in outs]


def test_darknet_graph_analysis_shapes_concat_layout_and_guards(tmp_path):
    """yolo/lower.py analyse() is a pure host function of the cfg: its per-section (C, H, W) against the stock nn modules run on the CPU,
    its concat layout (every producer's slice tiles the route buffer in `layers=` order, no overlap), and its two guards."""
    from mdcv.yolo.models import Darknet
    from mdcv.yolo.lower import analyse
    from mdcv.engine import pad8
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_models import write_baseline_cfg

    def build(cfg, where):
        cwd = os.getcwd()
        os.chdir(where)
        try:
            return Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True)
        finally:
            os.chdir(cwd)
    full = write_baseline_cfg(str(tmp_path), 416, 80)
    cases = [(n + ".cfg", os.path.join(G, "mini"), 64) for n in ("mini", "mini_tiny", "mini_relu")] + [(full, str(tmp_path), 416)]
    multi = 0
    for cfg, where, size in cases:
        net = build(cfg, where)
        defs = net.module_defs
        lay = analyse(defs, net.module_list, int(net.hyperparams["channels"]), size, size)
        assert lay.shp == _reference_shapes(net, size), cfg
        assert len(lay.users) == len(defs)
        for r, (ctot, parts) in lay.concat.items():
            src = [r + int(t) if int(t) < 0 else int(t) for t in defs[r]["layers"].split(",")]
            assert [s for s, _, _ in parts] == src and len(src) > 1
            off = 0
            for s, o, wd in parts:                           # consecutive slices, each as wide as its padded source
                assert o == off and wd == pad8(lay.shp[s][0])
                off += wd
            assert off == ctot and ctot >= lay.shp[r][0]
            assert all(r in lay.users[s] for s in src)
            multi += 1
        for s, (r, o) in lay.dest.items():                   # an in-place producer owns exactly one of those slices
            assert (s, o, pad8(lay.shp[s][0])) in lay.concat[r][1]
            assert defs[s]["type"] in ("convolutional", "upsample", "shortcut", "maxpool")
    assert multi >= 5                                        # 2 in yolo_baseline, at least one per mini cfg
    # the two guards, on cfgs derived from mini.cfg's header
    head = open(os.path.join(G, "mini", "mini.cfg")).read().split("[convolutional]")[0]

    def conv(f, k):
        return f"[convolutional]\nfilters={f}\nsize={k}\nstride=1\n\n"
    bad_route = head + conv(12, 3) + conv(16, 3) + "[route]\nlayers=-2, -1\n\n" + conv("preyolo", 1) + "[yolo]\n"
    bad_pool = head + conv(16, 3) + "[maxpool]\nsize=17\nstride=1\n\n" + conv("preyolo", 1) + "[yolo]\n"
    for text, msg in ((bad_route, r"\[route\] at section 2: source 0 has 12 channels; every concat source but the last must have a multiple of 8 channels"),
                      (bad_pool, "max-pool windows up to 15x15 are lowered")):
        cfg = tmp_path / "bad.cfg"
        cfg.write_text(text)
        net = build(str(cfg), os.path.join(G, "mini"))       # (dataset/train.csv is looked up relative to the working directory)
        with pytest.raises(NotImplementedError, match=msg):
            analyse(net.module_defs, net.module_list, 3, 64, 64)
