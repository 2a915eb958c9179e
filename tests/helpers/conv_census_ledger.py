"""The ledger of tests/test_gpu_conv_exact.py: test id -> the full set of convolution-kernel instantiations the case launched, recorded on the
MI355X.  The exact suite asserts that what it launches today EQUALS its entry, so a dispatch change that moves a case onto another instantiation
fails there and forces someone to look (and to run the command below) instead of passing silently; tests/test_gpu_conv_census.py asserts that
every instantiation the production plans launch is in the union of these sets (or on WAIVED).

Regenerate (on the GPU machine, from the repository root) with

    python tests/helpers/conv_census_ledger.py --regenerate

which runs the exact suite with MDCV_CENSUS_RECORD set (each test then appends what it launched to that file instead of comparing with its entry;
purpose patterns are still asserted) and rewrites tests/golden/conv_census_ledger.json.  Read the diff before committing it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_census as KC  # noqa: E402

DATA = os.path.join(os.path.dirname(HERE), "golden", "conv_census_ledger.json")
REGENERATE = "python tests/helpers/conv_census_ledger.py --regenerate"

# Production instantiations no exact case reaches under the reference cap (helpers/conv_exact.py DENSE_MACS_CAP).  Each entry: the instantiation as the
# ledger spells it -> (smallest geometry that reaches it, why the integer reference cannot afford it, the tolerance test that runs it at real size).
# Conditions (tests/test_conv_census_host.py): nothing the 416^2 B = 32 training step launches from the shift, pw_block, pw_bwd or stream families,
# and at most one tenth of the distinct bf16 production instantiations.
WAIVED = {}


def spell(inst):
    """(name, args) -> 'name<a, b, ...>' as a demangler prints it (bools as true / false)"""
    name, args = inst
    return name + ("<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args) + ">" if args else "")


def _load():
    if not os.path.exists(DATA):
        return {}
    with open(DATA) as f:
        return {k: frozenset(KC.parse(s) for s in v) for k, v in json.load(f).items()}


LEDGER = _load()


def union():
    out = set()
    for v in LEDGER.values():
        out |= v
    return out


def covering(inst):
    """the ids of the exact cases whose entry holds `inst`"""
    return [k for k, v in LEDGER.items() if inst in v]


def check(test_id, seen):
    """the observed set must equal the entry; with MDCV_CENSUS_RECORD set the observation is appended to that file instead"""
    rec = os.environ.get("MDCV_CENSUS_RECORD")
    seen = frozenset(seen)
    if rec:
        with open(rec, "a") as f:
            f.write(json.dumps({"id": test_id, "inst": sorted(spell(i) for i in seen)}) + "\n")
        return
    assert test_id in LEDGER, f"{test_id}: no ledger entry; it launched {sorted(map(spell, seen))}.  Regenerate the ledger: {REGENERATE}"
    want = LEDGER[test_id]
    if seen != want:
        gone, new = sorted(map(KC.show, want - seen)), sorted(map(KC.show, seen - want))
        raise AssertionError(f"{test_id} no longer runs the instantiations its ledger entry records (a dispatch change moved the case).\n"
                             f"  recorded, not launched now: {gone}\n  launched now, not recorded:  {new}\n"
                             f"  If the move is intended, check that the case still serves its purpose and regenerate the ledger: {REGENERATE}")


def _regenerate():
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(HERE))
    fd, path = tempfile.mkstemp(suffix=".jsonl")
    os.close(fd)
    rc = subprocess.call([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(root, "tests", "test_gpu_conv_exact.py")],
                         cwd=root, env=dict(os.environ, MDCV_CENSUS_RECORD=path), timeout=1200)     # (the suite takes well under a minute)
    write_from(path)
    os.unlink(path)
    return rc


def write_from(records):
    out = {}
    with open(records) as f:
        for line in f:
            r = json.loads(line)
            out[r["id"]] = sorted(set(out.get(r["id"], [])) | set(r["inst"]))
    with open(DATA, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(out.items())) + "\n}\n")
    print(f"{len(out)} entries written to {DATA}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--regenerate"]:
        sys.exit(_regenerate())
    if sys.argv[1:2] == ["--from"] and len(sys.argv) == 3:
        write_from(sys.argv[2])
        sys.exit(0)
    sys.exit(f"usage: {REGENERATE}")
