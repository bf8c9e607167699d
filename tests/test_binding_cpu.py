"""CPU tier of the binding (nero_amd/_lib.py): ONE list of public headers, _lib.HEADER_PATHS, is what parse_headers() and bind() read by
default, so the package's handle and a fresh bind(CDLL(path)) carry the same signature for every entry point.  TABLE below states, per
header, every entry point and its parameter count; the counts are checked against a prototype reader of this file's own, the handles
against the table, and the exact types wherever a narrower one would truncate a size, a count or a seed.

A new header: put it in include/, add its name to _lib.HEADER_PATHS, add a row to TABLE."""
import ctypes as C
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
FIRST = 'nero_hip.h'
N_FIRST, N_FIRST_SIZED, N_FIRST_VOID = 172, 24, 2          # nero_hip.h: its prototypes, those that return a size_t, those that return nothing
# header -> {entry point: parameter count}, in the order of _lib.HEADER_PATHS; the first header by its numbers above
TABLE = {
    FIRST: None,
    'nero_hip_visibility.h': {'nero_bvh_occluded': 9, 'nero_ao_rays': 10, 'nero_bvh_ao': 11},
    'nero_hip_relight.h': {'nero_bvh_export_faces': 2, 'nero_bvh_trace_faces': 8, 'nero_env_lookup': 10, 'nero_relight_rays': 11,
                           'nero_relight_workspace_bytes': 3, 'nero_bvh_relight': 20},
    'nero_hip_surface.h': {'nero_surface_cdf_workspace_bytes': 1, 'nero_surface_cdf': 8, 'nero_surface_sample': 16},
    'nero_hip_envsample.h': {'nero_env_cdf_workspace_bytes': 2, 'nero_env_cdf': 11, 'nero_relight_mis_rays': 20,
                             'nero_relight_mis_workspace_bytes': 4, 'nero_bvh_relight_mis': 25},
    'nero_hip_bounce.h': {'nero_relight_bounce_workspace_bytes': 3, 'nero_relight_mis_bounce_workspace_bytes': 4, 'nero_bvh_relight_bounce': 28,
                          'nero_bvh_relight_mis_bounce': 33, 'nero_relight_bounce_rays': 31},
    'nero_hip_normals.h': {'nero_vertex_normals_workspace_bytes': 2, 'nero_vertex_normals': 9},
    'nero_hip_denoise.h': {'nero_denoise_max_pixels': 0, 'nero_denoise_variance': 10, 'nero_denoise_atrous': 12},
    'nero_hip_texfetch.h': {'nero_tex_mip_levels': 2, 'nero_tex_mip_bytes': 2, 'nero_tex_pack': 7, 'nero_tex_mip_build': 4,
                            'nero_tex_face_scale': 11, 'nero_tex_materials': 18, 'nero_tex_vertex_materials': 13},
}
LATER = [h for h in TABLE if h != FIRST]
N_ALL = N_FIRST + sum(len(TABLE[h]) for h in LATER)
p, i, u, i64, f, sz = C.c_void_p, C.c_int, C.c_uint, C.c_int64, C.c_float, C.c_size_t
# entry point -> its whole argtypes
WHOLE = {
    'nero_check_device_memory': [sz, sz, C.c_char_p],
    'nero_surface_cdf_workspace_bytes': [i64],
    'nero_vertex_normals_workspace_bytes': [i64, i64],
    'nero_denoise_variance': [p, i, p, i64, i64, i, f, f, p, p],
    'nero_denoise_atrous': [p, i, p, i64, i64, i, i, f, f, f, p, p],
    'nero_tex_materials': [p, i64, i64, p, p, i64, p, i64, p, p, p, p, i64, f, f, p, p, p],
    'nero_tex_vertex_materials': [p, i64, i64, p, p, i64, p, p, i64, i64, p, p, p],
}
# entry point -> {parameter index: type}
AT = {
    'nero_ao_rays': {5: u},
    'nero_bvh_occluded': {5: f},
    'nero_env_lookup': {6: i64, 7: f},
    'nero_bvh_relight': {13: f, 18: sz},
    'nero_surface_sample': {1: i64, 3: i64, 6: i64, 7: i64, 8: i64, 9: u, 10: i},
    'nero_env_cdf': {5: f},
    'nero_bvh_relight_mis': {23: sz},
    'nero_bvh_relight_bounce': {13: f, 26: sz},
    'nero_bvh_relight_mis_bounce': {31: sz},
    'nero_relight_bounce_rays': {16: i},
    'nero_vertex_normals': {0: p, 1: i64, 3: i64, 4: i, 8: p},
}


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def fresh(L):
    """what bind() alone gives, whatever was imported"""
    return L.bind(C.CDLL(L.LIB_PATH))


def _prototypes(header):
    """{name: (return type, parameter count)} read off a header by this file's own rule, which shares nothing with _lib.parse_header:
    comments out, then `type name(params);`, a parameter per comma"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r'([\w ]+?[\s*]+)(nero_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text):
        protos[name] = (' '.join(ret.replace('*', ' * ').split()), 0 if params.strip() in ('', 'void') else params.count(',') + 1)
    return protos


def _counts(L, header):
    """{entry point: parameter count} of a header as the table has it; the first header's as this file reads them"""
    return TABLE[header] if TABLE[header] is not None else {n: c for n, (_, c) in _prototypes(header).items()}


def test_one_list_names_every_header_under_include(L):
    assert [os.path.basename(h) for h in L.HEADER_PATHS] == list(TABLE)
    assert set(L.HEADER_PATHS) == set(glob.glob(os.path.join(INCLUDE, 'nero_hip*.h')))        # a header left off the list fails here
    assert L.HEADER_PATHS[0] == L.HEADER_PATH
    assert len(L.parse_headers()) == N_ALL == 206
    assert L.parse_headers() == L.parse_headers(L.HEADER_PATHS)


@pytest.mark.parametrize('header', list(TABLE))
def test_a_header_declares_what_the_table_says(L, header):
    protos = _prototypes(header)
    if header == FIRST:
        names = sorted(set(re.findall(r'\b(nero_[a-z0-9_]+)\s*\(', open(L.HEADER_PATH).read())))   # the rule of tests/test_cabi.py: comments and all
        assert sorted(protos) == names and len(names) == N_FIRST
        assert len([n for n in names if protos[n][0] == 'size_t']) == N_FIRST_SIZED and len([n for n in names if protos[n][0] == 'void']) == N_FIRST_VOID
    else:
        assert {n: c for n, (_, c) in protos.items()} == TABLE[header]
    want = _counts(L, header)
    mine = {n: s for n, s in L.parse_headers().items() if s[2] == header}
    alone = L.parse_headers((os.path.join(INCLUDE, header),))
    assert {n: len(s[1]) for n, s in mine.items()} == want == {n: len(s[1]) for n, s in alone.items()}
    assert set(alone) == set(L.parse_header(open(os.path.join(INCLUDE, header)).read()))


def test_every_entry_point_is_bound_on_the_loaded_and_on_a_fresh_handle(L, fresh):
    exported = C.CDLL(L.LIB_PATH)
    assert fresh is not L.lib
    n = 0
    for header in TABLE:
        for name, n_par in _counts(L, header).items():
            assert hasattr(exported, name), name
            for lib in (fresh, L.lib):
                fn = getattr(lib, name)
                assert fn.argtypes is not None and len(fn.argtypes) == n_par, (name, fn.argtypes)
            assert getattr(fresh, name).argtypes == getattr(L.lib, name).argtypes and getattr(fresh, name).restype is getattr(L.lib, name).restype
            n += 1
    assert n == N_ALL


def test_result_types(L, fresh):
    for lib in (fresh, L.lib):
        for header in LATER:
            for name in TABLE[header]:
                want = sz if name.endswith('_workspace_bytes') or name == 'nero_tex_mip_bytes' else i64 if name == 'nero_denoise_max_pixels' else i
                assert getattr(lib, name).restype is want, name
        protos = _prototypes(FIRST)
        names = sorted(protos)
        assert [n for n in names if getattr(lib, n).restype is sz] == [n for n in names if protos[n][0] == 'size_t']
        assert [n for n in names if getattr(lib, n).restype is None] == [n for n in names if protos[n][0] == 'void']
        assert lib.nero_last_error.restype is C.c_char_p
        assert lib.nero_denoise_max_pixels() == 2 ** 31 - 1


def test_exact_argument_types(L, fresh):
    for lib in (fresh, L.lib):
        for name, want in WHOLE.items():
            assert getattr(lib, name).argtypes == want, name
        for name, at in AT.items():
            for k, want in at.items():
                assert getattr(lib, name).argtypes[k] is want, (name, k)


def test_a_name_declared_twice_is_refused(L, tmp_path):
    dup = tmp_path / 'dup.h'
    dup.write_text('int nero_fresh(int n);\nint nero_version(void);\n')
    with pytest.raises(ImportError, match='nero_version'):
        L.parse_headers((L.HEADER_PATH, str(dup)))
    assert 'nero_fresh' in L.parse_headers((str(dup),))


@pytest.mark.parametrize('header', list(TABLE))
def test_a_header_listed_twice_is_refused(L, header):
    with pytest.raises(ImportError) as e:                             # a name twice across ANY two entries of the list
        L.parse_headers(L.HEADER_PATHS + (os.path.join(INCLUDE, header),))
    m = re.fullmatch(rf'{re.escape(header)} declares (nero_\w+), which {re.escape(header)} declares already', str(e.value))
    assert m and m.group(1) in _counts(L, header), str(e.value)


def test_a_refusal_names_the_header_it_read(L, tmp_path):
    wide = tmp_path / 'wide.h'
    wide.write_text('int nero_wide(long double x, int n);\n')
    with pytest.raises(ImportError, match=r'^wide\.h: nero_wide: .*long double'):
        L.parse_headers((str(wide),))


def test_the_modules_carry_no_binding_of_their_own(L):
    from nero_amd import relight, surface
    for mod in (relight, surface):
        assert not hasattr(mod, 'SIGNATURES') and not hasattr(mod, 'HEADER_PATH') and not hasattr(mod, '_bind')
    src = open(surface.__file__).read()
    assert 'environ' not in src and 'getenv' not in src                # the module reads no environment variable


@pytest.mark.parametrize('header', list(TABLE))
def test_a_newer_public_header_makes_the_library_stale(L, header):
    """build()'s own predicate: every public header is a dependency of the library"""
    import __graft_entry__ as ge
    assert not ge.library_is_stale()
    path = os.path.join(INCLUDE, header)
    st = os.stat(path)
    try:
        os.utime(path, ns=(st.st_atime_ns, os.stat(ge.LIB).st_mtime_ns + 10 ** 9))
        assert ge.library_is_stale()
    finally:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not ge.library_is_stale()
