"""Which template instantiation ran: the in-library profiler (mdcv_profile_begin / _stop / _read, csrc/runtime.hip) returns the demangled symbol of
every kernel the library launches, template arguments included.  `launched(L)` collects them around a block of calls, `parse` splits a symbol into
(kernel name, template arguments), `PARAMS` names the arguments as the declarations in csrc/ do, so that a pattern such as {"BM": 384} or
{"BRING": 3, "LOOP": 0} can be matched against what ran (tests/test_gpu_conv_exact.py, tests/test_gpu_conv_census.py).

Importing this file needs neither a GPU nor the library."""
import contextlib
import ctypes
import fnmatch

NAME_BYTES = 1024                 # as engine.run_timed reads them; a conv symbol does not fit the 256 bytes the data-loader tests use

# the census's scope: the convolution kernel families (fnmatch patterns on the parsed kernel name)
CONV_FAMILIES = ("conv_igemm_kernel", "conv_glds_kernel", "mdcv_conv3x3_shift_kernel", "conv_wgrad_kernel", "conv_wgrad_dma_kernel",
                 "conv_wgrad_dma_narrow_kernel", "wgrad3x3_stream_kernel", "wgrad3x3_s2_stream_kernel", "wgrad3x3_shift_kernel", "wgrad7x7_stream_kernel",
                 "wgrad_reduce*_kernel", "pw_block_kernel", "pw_bwd_kernel", "first_conv_kernel")

# template parameter names, copied from the declarations (file: line of the `template <...>` above the __global__)
PARAMS = {
    "conv_igemm_kernel": ("T", "MODE", "BM", "BN", "WM", "WN", "KT"),                                                     # conv_gemm.h:94
    "conv_glds_kernel": ("T", "MODE", "BM", "BN", "WM", "WN", "STAGES", "UT", "FUSE", "EPI", "ALLCLS"),                   # conv_gemm.h:384
    "mdcv_conv3x3_shift_kernel": ("MODE", "BM", "NPA", "BRING", "FUSE", "WN", "EPI", "BN", "LOOP"),                       # conv_shift.hip:76 (BN_ there)
    "conv_wgrad_kernel": ("T",),                                                                                           # wgrad_gemm.hip:29
    "conv_wgrad_dma_kernel": ("BP", "STAGES", "SAME"),                                                                     # wgrad_gemm.hip:196
    "conv_wgrad_dma_narrow_kernel": ("SAME", "STAGES", "BNA"),                                                             # wgrad_gemm.hip:389
    "wgrad3x3_stream_kernel": ("NCI", "NCO", "A", "PG", "BP", "D", "TGRP", "TILED", "NW", "TBL", "DIRECT"),               # wgrad_stream.hip:97
    "wgrad3x3_s2_stream_kernel": ("D",),                                                                                   # wgrad_stream_s2.hip:67
    "wgrad3x3_shift_kernel": (),
    "wgrad7x7_stream_kernel": (),
    "wgrad_reduce_kernel": (),
    "wgrad_reduce_kk_kernel": ("KK",),                                                                                     # wgrad_reduce.hip:44
    "wgrad_reduce_flat_kernel": (),
    "pw_block_kernel": ("BMP", "FNW", "NV", "HASR", "WRES"),                                                               # pw_block.hip:53
    "pw_bwd_kernel": ("CO4", "S", "ADD", "FUSE"),                                                                          # pw_bwd.hip:60
    "first_conv_kernel": ("MODE",),                                                                                        # first_conv.hip:33
}


def _split_top(s, sep=","):
    """split on `sep` outside every <>, () and []"""
    out, depth, cur = [], 0, []
    for ch in s:
        if ch in "<([":
            depth += 1
        elif ch in ">)]":
            depth -= 1
        if ch == sep and depth == 0:
            out.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    tail = "".join(cur).strip()
    if tail or out:
        out.append(tail)
    return out


def _value(tok):
    """a template argument as Python: bools and integers (with the suffixes a demangler may print) as such, everything else (types) as text"""
    if tok in ("true", "false"):
        return tok == "true"
    t = tok
    if t.startswith("(") and ")" in t:                    # "(int)3", "(bool)1": the cast form older demanglers print
        t = t[t.index(")") + 1:]
    t = t.rstrip("uUlL")
    try:
        return int(t)
    except ValueError:
        return tok


def parse(symbol):
    """'void (anonymous namespace)::k<unsigned short, 1, true>(Args, unsigned int)' -> ('k', ('unsigned short', 1, True))"""
    s = symbol.strip()
    if s.startswith("void "):
        s = s[5:]
    if s.endswith(")"):                                    # the parameter list: from the '(' that matches the last ')'
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += s[i] == ")"
            depth -= s[i] == "("
            if depth == 0:
                s = s[:i]
                break
    s = s.strip()
    args = ()
    if s.endswith(">"):                                    # the template arguments: from the '<' that matches the last '>'
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += s[i] == ">"
            depth -= s[i] == "<"
            if depth == 0:
                args = tuple(_value(t) for t in _split_top(s[i + 1:-1]))
                s = s[:i]
                break
    return s.rsplit("::", 1)[-1].strip(), args


def in_scope(name):
    return any(fnmatch.fnmatchcase(name, f) for f in CONV_FAMILIES)


def named(inst):
    """(name, args) -> {parameter name: value} by PARAMS (a missing trailing argument is absent, an unknown kernel has positional names)"""
    name, args = inst
    names = PARAMS.get(name)
    if names is None:
        names = tuple(f"arg{i}" for i in range(len(args)))
    assert len(args) <= len(names), f"{name}: {len(args)} template arguments, PARAMS names {len(names)}"
    return dict(zip(names, args))


def matches(inst, pattern):
    """pattern: (names, {parameter: value}) where `names` is a kernel name, an fnmatch pattern, or a tuple of either; the kernel must match one of the
    names, and every named parameter must be present and equal (a bool is not an integer)"""
    kname, want = pattern
    if not any(fnmatch.fnmatchcase(inst[0], k) for k in ((kname,) if isinstance(kname, str) else kname)):
        return False
    have = named(inst)
    return all(k in have and have[k] == v and type(have[k]) is type(v) for k, v in want.items())


def show(inst):
    name, args = inst
    nm = named(inst)
    return name + ("<" + ", ".join(f"{k}={str(v).lower() if isinstance(v, bool) else v}" for k, v in nm.items()) + ">" if args else "")


def conv_instantiations(symbols):
    """the parsed CONV_FAMILIES instantiations of a list of symbols, in launch order (with repeats)"""
    out = [parse(s) for s in symbols]
    return [i for i in out if in_scope(i[0])]


@contextlib.contextmanager
def launched(L):
    """with launched(L) as syms: ...   -- afterwards `syms` holds the demangled symbol of every kernel the library launched inside the block"""
    import torch
    syms = []
    torch.cuda.synchronize()
    rc = L.profile_begin()
    assert rc == 0, f"mdcv_profile_begin returned {rc}"
    try:
        yield syms
    finally:
        torch.cuda.synchronize()
        n = L.profile_stop()
        assert n >= 0, f"mdcv_profile_stop returned {n}"
        buf, ms = ctypes.create_string_buffer(NAME_BYTES), ctypes.c_float()
        for i in range(n):
            rc = L.profile_read(i, ctypes.byref(ms), buf, NAME_BYTES)
            assert rc == 0, f"mdcv_profile_read({i}) returned {rc}"
            syms.append(buf.value.decode())
