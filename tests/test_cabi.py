"""CPU tier: the C-ABI library loads and exports every symbol include/nero_hip.h declares (no compute calls); that every entry point of
every header is bound: tests/test_binding_cpu.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(ROOT, 'include', 'nero_hip.h')).read()
    names = sorted(set(re.findall(r'\b(nero_[a-z0-9_]+)\s*\(', hdr)))
    assert len(names) >= 30
    lib = ctypes.CDLL(os.path.join(ROOT, 'nero_amd', 'libnero_hip.so'))
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.nero_last_error.restype = ctypes.c_char_p
    assert lib.nero_version() >= 100
    assert isinstance(lib.nero_last_error(), bytes)


# (C struct, ctypes mirror as 'module.Class') of every struct include/nero_hip.h defines.  stage1.Linear / stage2.Weights appear twice: the
# package fills the gradient tables through the mirrors of the weight tables (same layout).
STRUCTS = (('nero_fwd_layer', '_lib.FwdLayer'), ('nero_fwd_chain', '_lib.FwdChain'), ('nero_tan_layer', '_lib.TanLayer'),
           ('nero_tan_chain', '_lib.TanChain'), ('nero_bwd_layer', '_lib.BwdLayer'), ('nero_bwd_chain', '_lib.BwdChain'),
           ('nero_dw_job', '_lib.DwJob'), ('nero_pack_job', '_lib.PackJob'), ('nero_wn_job', '_lib.WnJob'),
           ('nero_wn_grad_job', '_lib.WnGradJob'), ('nero_adam_job', '_lib.AdamJob'),
           ('nero_linear', 'stage1.Linear'), ('nero_linear_grad', 'stage1.Linear'), ('nero_stage1_weights', 'stage1.Weights'),
           ('nero_stage1_grads', 'stage1.Grads'), ('nero_stage1_cfg', 'stage1.Cfg'), ('nero_stage1_state', 'stage1.State'),
           ('nero_stage2_weights', 'stage2.Weights'), ('nero_stage2_grads', 'stage2.Weights'), ('nero_stage2_cfg', 'stage2.Cfg'),
           ('nero_mat_loss_cfg', 'stage2.LossCfg'))
# the fields whose Python name is not the header's: (C struct, Python field, C field)
RENAMED_FIELDS = (('nero_linear_grad', 'W', 'dW'), ('nero_linear_grad', 'b', 'db'))


def test_struct_layouts_match_header():
    """ctypes mirrors of the header's structs must have the sizes the C compiler gives them, and every field the offset of the header's
    field of the same name (RENAMED_FIELDS: of the field it stands for); the list covers every struct the header defines"""
    import importlib, subprocess, tempfile
    hdr = open(os.path.join(ROOT, 'include', 'nero_hip.h')).read()
    defined = set(re.findall(r'^\}\s*(nero_\w+);', hdr, re.M)) | set(re.findall(r'^typedef struct \{.*\}\s*(nero_\w+);', hdr, re.M))
    assert defined == {c for c, _ in STRUCTS}, defined ^ {c for c, _ in STRUCTS}
    renamed = {(c, p): f for c, p, f in RENAMED_FIELDS}
    lines, mine = [], []
    for cname, path in STRUCTS:
        mod, cls = path.split('.')
        t = getattr(importlib.import_module('nero_amd.' + mod), cls)
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        mine.append((cname, 'sizeof', ctypes.sizeof(t)))
        for name, _ in t._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {renamed.get((cname, name), name)}));')
            mine.append((cname, name, getattr(t, name).offset))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nero_hip.h"\nint main(){\n' + '\n'.join(lines) + '\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 's.c')
        open(c, 'w').write(src)
        exe = os.path.join(td, 's')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        theirs = [int(x) for x in subprocess.check_output([exe]).split()]
    assert len(theirs) == len(mine)
    wrong = [(m, t) for m, t in zip(mine, theirs) if m[2] != t]
    assert not wrong, wrong


def test_dw_workspace_is_worst_case_sized():
    """regression: the split-K slice count is not monotonic in the row count, so the workspace query must not depend on it"""
    lib = ctypes.CDLL(os.path.join(ROOT, 'nero_amd', 'libnero_hip.so'))
    base = 256 * (256 * 256 + 256)
    for n in (0, 1, 100, 8000, 8192, 8193, 300000, 1 << 22):
        assert lib.nero_dw_workspace_floats(n) >= base
    assert lib.nero_dw_workspace_floats(1 << 22) >= ((1 << 22) // 128) * 1028


def test_f16_paired_selector_round_trip():
    """nero_f16_paired (no GPU needed: a host-side selection): a negative mask only queries, a mask is kept modulo its four bits, the call
    returns the previous selection; the default is forward + tangent (3) unless NERO_F16_PAIRED says otherwise"""
    from nero_amd import chain as CH
    prev = CH.f16_paired()
    try:
        if 'NERO_F16_PAIRED' not in os.environ:
            assert prev == 3
        assert CH.f16_paired(8 | 5) == prev
        assert CH.f16_paired() == 13
        assert CH.f16_paired(0x47) == 13              # only bits 0-3 are kept
        assert CH.f16_paired(-1) == 7
    finally:
        CH.f16_paired(prev)
    assert CH.f16_paired() == prev


def test_signatures_are_live():
    """a float is not taken for an int, and an int64_t above 2^32 reaches C whole.  No host-only size query quotes its argument in its refusal,
    so this is the second variant: (2^33 + 7) triangles are refused for their RANGE, where 7 -- what a 32-bit pass of the same number leaves --
    yields a size, or on a machine without a device the refusal that names the failed scratch `query` (tests/test_host_logic.py)"""
    import pytest
    from nero_amd import _lib as L
    with pytest.raises(ctypes.ArgumentError):
        L.lib.nero_dw_workspace_floats(1.5)
    fn = L.lib.nero_uv_raster_workspace_bytes
    small = fn(7)
    assert small > 0 or b'query' in L.lib.nero_last_error()
    assert fn((1 << 33) + 7) == 0
    err = L.lib.nero_last_error()
    assert b'nt must be in [0, 2^31 - 1)' in err and b'query' not in err, err


def test_the_parser_refuses_what_it_does_not_know():
    import pytest
    from nero_amd import _lib as L
    ok = L.parse_header('int nero_fine(const float* x /*[n]*/, int64_t n, void* stream);  // size_t nero_not_there(int n);\n')
    assert ok == {'nero_fine': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])}
    with pytest.raises(ImportError, match='nero_wide.*long double'):
        L.parse_header('int nero_fine(int n);\nint nero_wide(long double x, int n);\n')
    with pytest.raises(ImportError, match='nero_callback'):             # named, but not a prototype the parser reads
        L.parse_header('int nero_fine(int n);\nint nero_callback(int (*f)(int));\n')
    with pytest.raises(ImportError, match='does not export nero_'):       # a library without a declared symbol
        L.bind(object())


def test_signatures_are_declared_in_one_place():
    """the two words appear in _lib.py alone -- as an attribute, a string handed to setattr, or prose"""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, 'nero_amd', '*.py'))):
        hits = re.findall(r'.*(?:argtypes|restype).*', open(path).read())
        assert bool(hits) == (os.path.basename(path) == '_lib.py'), (path, hits)
