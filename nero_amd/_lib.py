"""ctypes binding of libnero_hip.so: every public header under include/ (HEADER_PATHS, EXTRA_HEADER_PATHS, NEWER_HEADER_PATHS) is bound here and
nowhere else.  The library is
REQUIRED: there is no PyTorch/CPU fallback for the product path -- if it is missing or fails to load, importing this module raises."""
import ctypes as C
import os
import re

import torch  # noqa: F401  -- must come first: libnero_hip.so has to bind to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NERO_HIP_LIB') or os.path.join(_HERE, 'libnero_hip.so')     # (override: kernel-variant experiments)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'nero_hip.h')
# every public header of the library, in the order they were added: the ONE list.  An entry point is declared in exactly one of them, and
# parse_headers() and bind() read all of them unless told otherwise.  A new header goes into include/ and into this tuple
HEADER_PATHS = tuple(os.path.join(os.path.dirname(HEADER_PATH), h)
                     for h in ('nero_hip.h', 'nero_hip_visibility.h', 'nero_hip_relight.h', 'nero_hip_surface.h', 'nero_hip_envsample.h',
                               'nero_hip_bounce.h', 'nero_hip_normals.h', 'nero_hip_denoise.h', 'nero_hip_texfetch.h'))
# headers added since the binding test (tests/test_binding_cpu.py, which pins HEADER_PATHS to the nero_hip*.h files and their entry points)
# was last touched: bound by _load() after the first list, with the same parser.  Folding the two lists into one belongs to whichever later
# change may edit that test; until then a header here must not match nero_hip*.h
EXTRA_HEADER_PATHS = tuple(os.path.join(os.path.dirname(HEADER_PATH), h) for h in ('nero_closest.h',))
# ... and since tests/test_closest_point_cpu.py pinned the second list to that one header: a third list, bound after the other two, under the
# same rule.  A new header goes HERE until a change that may edit both tests folds the three lists into one
NEWER_HEADER_PATHS = tuple(os.path.join(os.path.dirname(HEADER_PATH), h) for h in ('nero_transfer.h',))

MAX_LAYERS = 10
HID = 256
ACT_NONE, ACT_RELU, ACT_SOFTPLUS100 = 0, 1, 2
GEMM_F32, GEMM_BF16X6, GEMM_F16X3 = 0, 1, 2

_fp = C.c_void_p   # device pointers travel as integers


class FwdLayer(C.Structure):
    _fields_ = [('w_main', _fp), ('w_aux', _fp), ('bias', _fp), ('save', _fp), ('head_w', _fp), ('head_b', _fp),
                ('head_out', _fp), ('k_main', C.c_int), ('k_aux', C.c_int), ('n_tiles', C.c_int), ('n_head', C.c_int),
                ('act', C.c_int), ('head_k', C.c_int), ('relu_mask', _fp)]


class FwdChain(C.Structure):
    _fields_ = [('init', _fp), ('aux', _fp), ('ld_init', C.c_int), ('k_init', C.c_int), ('ld_aux', C.c_int),
                ('k_aux', C.c_int), ('n_layers', C.c_int), ('aux_wide', C.c_int), ('gemm_mode', C.c_int), ('pad_', C.c_int),
                ('macs_per_row', C.c_double), ('layer', FwdLayer * MAX_LAYERS)]


class TanLayer(C.Structure):
    _fields_ = [('w_main', _fp), ('w_aux', _fp), ('a_saved', _fp), ('gbar', _fp), ('adot', _fp), ('inj', _fp),
                ('k_main', C.c_int), ('k_aux', C.c_int), ('n_tiles', C.c_int), ('pad_', C.c_int)]


class TanChain(C.Structure):
    _fields_ = [('init', _fp), ('aux', _fp), ('ld_init', C.c_int), ('k_init', C.c_int), ('ld_aux', C.c_int),
                ('k_aux', C.c_int), ('n_layers', C.c_int), ('aux_wide', C.c_int), ('gemm_mode', C.c_int), ('pad_', C.c_int),
                ('macs_per_row', C.c_double), ('layer', TanLayer * MAX_LAYERS)]


class BwdLayer(C.Structure):
    _fields_ = [('w_main_t', _fp), ('w_aux_t', _fp), ('a_prev', _fp), ('inj', _fp), ('delta_prev', _fp),
                ('head_w', _fp), ('head_dy', _fp), ('n_out', C.c_int), ('k_main_tiles', C.c_int),
                ('k_aux_tiles', C.c_int), ('n_head', C.c_int), ('act_prev', C.c_int), ('pad_', C.c_int), ('mask_prev', _fp), ('inj_adot', _fp)]


class BwdChain(C.Structure):
    _fields_ = [('dy', _fp), ('ld_dy', C.c_int), ('k_dy', C.c_int), ('d_init', _fp), ('d_aux', _fp),
                ('ld_dinit', C.c_int), ('ld_daux', C.c_int), ('accumulate_dinit', C.c_int), ('n_layers', C.c_int),
                ('aux_wide', C.c_int), ('gemm_mode', C.c_int), ('macs_per_row', C.c_double), ('layer', BwdLayer * MAX_LAYERS)]


class PackJob(C.Structure):
    _fields_ = [('W', _fp), ('out', _fp), ('kind', C.c_int), ('nrows', C.c_int), ('ld', C.c_int), ('col0', C.c_int),
                ('ncols', C.c_int), ('transpose', C.c_int), ('kpad', C.c_int), ('nt_count', C.c_int), ('scale', C.c_float),
                ('pad_', C.c_int)]


MAX_PACK_JOBS = 64


class DwJob(C.Structure):
    _fields_ = [('d0', _fp), ('b0', _fp), ('d1', _fp), ('b1', _fp), ('ldd0', C.c_int), ('ldb0', C.c_int),
                ('ldd1', C.c_int), ('ldb1', C.c_int), ('n_out', C.c_int), ('k_cols', C.c_int), ('dW', _fp),
                ('ldw', C.c_int), ('col0', C.c_int), ('db', _fp), ('scale', C.c_float), ('accumulate', C.c_int),
                ('gemm_mode', C.c_int), ('pad_', C.c_int)]


class WnJob(C.Structure):
    _fields_ = [('v', _fp), ('g', _fp), ('w_eff', _fp), ('inv_norm', _fp), ('v_rw', _fp), ('g_rw', _fp), ('dW', _fp), ('m_v', _fp),
                ('v_v', _fp), ('m_g', _fp), ('v_g', _fp), ('rows', C.c_int), ('cols', C.c_int)]


class WnGradJob(C.Structure):
    _fields_ = [('v', _fp), ('g', _fp), ('inv_norm', _fp), ('dW', _fp), ('dv', _fp), ('dg', _fp), ('rows', C.c_int), ('cols', C.c_int)]


class AdamJob(C.Structure):
    _fields_ = [('p', _fp), ('grad', _fp), ('m', _fp), ('v', _fp), ('n', C.c_int), ('step', C.c_int)]


MAX_WN_JOBS, MAX_ADAM_JOBS = 40, 96


_SCALARS = {'int': C.c_int, 'unsigned': C.c_uint, 'unsigned int': C.c_uint, 'int64_t': C.c_int64, 'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t}


def _ctype(decl, fn, ret=False):
    """ctypes type of one parameter declaration (or return type) of `fn`: `const char*` is c_char_p, every other pointer -- device or
    host, struct, handle or out-parameter -- travels as c_void_p (which takes None, data_ptr() integers, byref(), arrays and pointers)"""
    if '*' in decl:
        return C.c_char_p if re.fullmatch(r'const\s+char\s*\*(\s*\w+)?', decl) else C.c_void_p
    words = [w for w in decl.split() if w != 'const']
    ctype = ' '.join(words if ret or len(words) == 1 else words[:-1])       # a parameter's last word is its name
    if ret and ctype == 'void':
        return None
    if ctype not in _SCALARS:
        raise ImportError(f'{fn}: no ctypes type for {ctype!r} (in {decl!r})')
    return _SCALARS[ctype]


def parse_header(text):
    """{function: (restype, argtypes)} for every prototype in `text`, the contents of one public header; parse_headers puts the file's
    name in front of what this refuses"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*|^\s*#[^\n]*', ' ', text, flags=re.S | re.M)       # comments, preprocessor lines
    sigs = {}
    for ret, fn, params in re.findall(r'([\w\s*]+?)\b(nero_\w+)\s*\(([^()]*)\)\s*;', text):
        params = [p.strip() for p in params.split(',') if p.strip() not in ('', 'void')]
        sigs[fn] = (_ctype(ret.strip(), fn, ret=True), [_ctype(p, fn) for p in params])
    names = set(re.findall(r'\b(nero_\w+)\s*\(', text))
    if set(sigs) != names:
        raise ImportError(f'{len(sigs)} prototypes parsed, {len(names)} functions named: {sorted(names ^ set(sigs))}')
    return sigs


def parse_headers(paths=None):
    """{function: (restype, argtypes, header file name)} over all of `paths` (default HEADER_PATHS: every public header), each read by
    parse_header; a name that two headers declare is an ImportError"""
    sigs = {}
    for path in HEADER_PATHS if paths is None else paths:
        name = os.path.basename(path)
        with open(path) as f:
            try:
                parsed = parse_header(f.read())
            except ImportError as e:
                raise ImportError(f'{name}: {e}') from None
        for fn, (restype, argtypes) in parsed.items():
            if fn in sigs:
                raise ImportError(f'{name} declares {fn}, which {sigs[fn][2]} declares already')
            sigs[fn] = (restype, argtypes, name)
    return sigs


def bind(lib, paths=None):
    """set restype and argtypes of EVERY entry point the headers (`paths`, default HEADER_PATHS: all of them) declare on `lib` (a CDLL of
    libnero_hip.so): a header is the one place a signature is written, so a size_t, an int64_t or a pointer reaches C whole whatever the call
    site hands over"""
    for fn, (restype, argtypes, header) in parse_headers(paths).items():
        try:
            f = getattr(lib, fn)
        except AttributeError:
            raise ImportError(f'{getattr(lib, "_name", lib)} does not export {fn}, which {header} declares: rebuild the library') from None
        f.restype, f.argtypes = restype, argtypes
    return lib


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          f'(hipcc --offload-arch=gfx950).  nero_amd has no non-HIP fallback.')
    return bind(bind(bind(C.CDLL(LIB_PATH)), EXTRA_HEADER_PATHS), NEWER_HEADER_PATHS)


lib = _load()


class NeroHipError(RuntimeError):
    pass


class NeroOutOfMemory(NeroHipError, MemoryError):
    """a step workspace larger than what the device can hold (NERO_ERR_NOMEM, nero_check_device_memory)"""


def check_workspace_fits(need_bytes, device, held_bytes=0, what='step workspace'):
    """raise NeroOutOfMemory -- with the byte counts -- BEFORE torch is asked for a workspace that cannot fit: free device memory + what torch's
    caching allocator holds without using + the caller's previous workspace (released for the new one) must cover it"""
    reusable = int(held_bytes)
    try:
        reusable += max(0, torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device))
    except Exception:                                  # noqa: BLE001 (no CUDA context yet)
        pass
    with torch.cuda.device(device):
        check(lib.nero_check_device_memory(int(need_bytes), reusable, what.encode()))


def check(rc):
    if rc != 0:
        msg = lib.nero_last_error().decode()
        if rc == -3:
            raise NotImplementedError(msg)
        if rc == -4:                                   # NERO_ERR_NOMEM: a workspace that cannot fit, reported BEFORE the allocation is tried
            raise NeroOutOfMemory(msg)
        raise NeroHipError(f'libnero_hip error {rc}: {msg}')


def ptr(t):
    """device pointer of a torch tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
