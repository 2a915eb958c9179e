"""No GPU: the kernel-census helper parses the symbols the in-library profiler returns; the ledger of tests/test_gpu_conv_exact.py
(helpers/conv_census_ledger.py) has an entry for exactly the ids that file parametrises, and every entry satisfies the purpose pattern of its
case (helpers/conv_exact.py purpose) -- so a ledger regenerated after a dispatch change cannot quietly record a case that no longer tests what
its comment says."""
import os
import pickle
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import conv_exact as X  # noqa: E402
import kernel_census as KC  # noqa: E402
import conv_census_ledger as LG  # noqa: E402

SYMBOLS = [
    # bool arguments, a trailing parameter list with spaces
    ("void mdcv_conv3x3_shift_kernel<0, 256, 3, 3, false, 2, false, 128, 0>(ShiftArgs, unsigned int, unsigned int)",
     ("mdcv_conv3x3_shift_kernel", (0, 256, 3, 3, False, 2, False, 128, 0))),
    # a type argument of two words, an anonymous-namespace prefix
    ("void (anonymous namespace)::conv_glds_kernel<unsigned short, 1, 128, 64, 2, 2, 3, true, true, false, false>((anonymous namespace)::ConvArgs, unsigned int, unsigned int)",
     ("conv_glds_kernel", ("unsigned short", 1, 128, 64, 2, 2, 3, True, True, False, False))),
    ("void mdcv::detail::conv_igemm_kernel<float, 0, 128, 128, 2, 2, 1>(mdcv::detail::ConvArgs)", ("conv_igemm_kernel", ("float", 0, 128, 128, 2, 2, 1))),
    # a type argument that is itself a template, nested commas
    ("void conv_wgrad_kernel<vec<unsigned short, 8> >(WgradArgs)", ("conv_wgrad_kernel", ("vec<unsigned short, 8>",))),
    # no template arguments; no `void`; a function-pointer parameter
    ("wgrad3x3_shift_kernel(WgradShiftArgs, unsigned int, unsigned int)", ("wgrad3x3_shift_kernel", ())),
    ("void wgrad_reduce_kk_kernel<9>(float const*, float*, int, int, int, int, int, int, void (*)(int))", ("wgrad_reduce_kk_kernel", (9,))),
    # the cast form and integer suffixes some demanglers print
    ("void pw_bwd_kernel<(int)8, (int)3, (bool)1, false>(PwbArgs)", ("pw_bwd_kernel", (8, 3, 1, False))),
    ("void first_conv_kernel<1u>(FirstConvArgs)", ("first_conv_kernel", (1,))),
    ("kernel@0x7f00", ("kernel@0x7f00", ())),
]


@pytest.mark.parametrize("symbol,want", SYMBOLS, ids=[w[0] + str(i) for i, (_, w) in enumerate(SYMBOLS)])
def test_parse(symbol, want):
    assert KC.parse(symbol) == want


def test_patterns_and_scope():
    shift = KC.parse(SYMBOLS[0][0])
    assert KC.named(shift) == dict(MODE=0, BM=256, NPA=3, BRING=3, FUSE=False, WN=2, EPI=False, BN=128, LOOP=0)
    assert KC.matches(shift, ("mdcv_conv3x3_shift_kernel", {"BRING": 3, "LOOP": 0})) and not KC.matches(shift, ("mdcv_conv3x3_shift_kernel", {"BM": 384}))
    assert KC.matches(shift, (("conv_glds_kernel", "mdcv_conv3x3_shift_kernel"), {"MODE": 0})) and not KC.matches(shift, ("conv_glds_kernel", {}))
    assert not KC.matches(shift, ("mdcv_conv3x3_shift_kernel", {"FUSE": 0})), "a bool parameter is not matched by an integer"
    assert not KC.matches(KC.parse(SYMBOLS[4][0]), ("wgrad3x3_shift_kernel", {"BM": 1})), "a parameter the kernel does not have never matches"
    assert KC.matches(KC.parse(SYMBOLS[5][0]), ("wgrad_reduce*_kernel", {})) and KC.in_scope("wgrad_reduce_flat_kernel") and KC.in_scope("wgrad_reduce_kernel")
    assert not KC.in_scope("imgload_hpass_kernel") and not KC.in_scope("kernel@0x7f00")
    assert KC.show(shift) == "mdcv_conv3x3_shift_kernel<MODE=0, BM=256, NPA=3, BRING=3, FUSE=false, WN=2, EPI=false, BN=128, LOOP=0>"
    assert KC.parse(LG.spell(shift)) == shift, "the ledger's spelling parses back"
    assert [i[0] for i in KC.conv_instantiations([s for s, _ in SYMBOLS])] == [w[0] for _, w in SYMBOLS[:-1]]
    for name, params in KC.PARAMS.items():
        assert KC.in_scope(name) and len(set(params)) == len(params), name


_COLLECT = """
import pickle, sys, pytest
items = []
class Grab:
    def pytest_itemcollected(self, item):
        items.append((item.name, item.originalname, dict(item.callspec.params) if hasattr(item, "callspec") else {}))
rc = pytest.main(["--collect-only", "-q", "-p", "no:cacheprovider", sys.argv[1]], plugins=[Grab()])
pickle.dump((int(rc), items), open(sys.argv[2], "wb"))
"""


def exact_items(tmp):
    """(node name, function name, parameters) of every test tests/test_gpu_conv_exact.py parametrises: collected by pytest itself in a process of its
    own (nothing runs, and this session's plugins and capture are left alone)"""
    out = os.path.join(str(tmp), "items.pkl")
    subprocess.run([sys.executable, "-c", _COLLECT, os.path.join(HERE, "test_gpu_conv_exact.py"), out], cwd=os.path.dirname(HERE), check=True,
                   stdout=subprocess.DEVNULL, timeout=300)
    with open(out, "rb") as f:
        rc, items = pickle.load(f)
    assert rc == 0 and items, rc
    return [i for i in items if i[1] != "test_tables_are_the_kernel_file_tables"]


@pytest.fixture(scope="module")
def items(tmp_path_factory):
    return exact_items(tmp_path_factory.mktemp("collect"))


def test_every_case_has_a_purpose(items):
    for name, fn, params in items:
        need, forbid = X.purpose(fn, params)
        assert need, f"{name}: no pattern it must launch"
        for kname, want in need + forbid:
            known = [n for k in ((kname,) if isinstance(kname, str) else kname) for n in KC.PARAMS if KC.matches((n, ()), (k, {}))]
            assert known, f"{name}: pattern names no known kernel: {kname}"
            for prm in want:
                assert any(prm in KC.PARAMS[n] for n in known), f"{name}: none of {known} has a template parameter {prm}"


def test_ledger_ids_are_the_parametrisation(items):
    ids = {name for name, _, _ in items}
    assert len(ids) == len(items), "duplicate test ids"
    stale, missing = sorted(set(LG.LEDGER) - ids), sorted(ids - set(LG.LEDGER))
    assert not stale and not missing, f"stale ledger entries {stale[:8]} ({len(stale)}), tests without an entry {missing[:8]} ({len(missing)}): {LG.REGENERATE}"


def test_ledger_entries_satisfy_their_purpose(items):
    bad = []
    for name, fn, params in items:
        seen = LG.LEDGER.get(name, frozenset())
        need, forbid = X.purpose(fn, params)
        for pat in need:
            if not any(KC.matches(i, pat) for i in seen):
                bad.append(f"{name}: is there for {pat}, the ledger records {sorted(map(KC.show, seen))}")
        for pat in forbid:
            hit = [KC.show(i) for i in seen if KC.matches(i, pat)]
            if hit:
                bad.append(f"{name}: is there for a path without {pat}, the ledger records {hit}")
    assert not bad, "\n".join(bad[:20])


def test_tables_cover_what_their_rows_promise():
    """what a whole table is there for, where a single case cannot say it: the default-code shift cases (SHIFT_CASES, DENSE_CASES) run 256-, 128- and 192-row tiles between them, the
    stride-2 weight-gradient cases the three prefetch depths of the parity-plane kernel; every WAIVED entry is spelled as the ledger spells it"""
    def union(prefix):
        out = set()
        for k, v in LG.LEDGER.items():
            if k.startswith(prefix + "["):
                out |= v
        return out
    shift = union("test_b_shift_default") | union("test_i_dense_forward")     # (SHIFT_CASES grids are too small for 192-row tiles: DENSE_FWD runs them)
    for bm in (256, 128, 192):
        assert any(KC.matches(i, (X.SHIFT, {"BM": bm})) for i in shift), f"no default shift case runs {bm}-row tiles"
    s2 = union("test_e_wgrad_stride2")
    for d in (1, 2, 3):
        assert any(KC.matches(i, (X.WG_S2, {"D": d})) for i in s2), f"no stride-2 weight-gradient case runs prefetch depth {d}"
    for s in LG.WAIVED:
        assert LG.spell(KC.parse(s)) == s and s not in {LG.spell(i) for i in LG.union()}, s
