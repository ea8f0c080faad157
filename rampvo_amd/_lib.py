"""ctypes binding of libramp_hip.so (C ABI declared in include/ramp_hip.h).

There is no CPU fallback: every operator of this package runs its HIP kernel
or raises.  ``lib()`` raises ``RuntimeError`` if the shared library has not been
built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C rampvo_amd/csrc``).
"""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("RAMP_HIP_LIB") or os.path.join(CSRC, "libramp_hip.so")   # env: kernel A/B builds

HEADER = os.path.join(os.path.dirname(_HERE), "include", "ramp_hip.h")

_C_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "const char *": ctypes.c_char_p}
_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "long": ctypes.c_long,
              "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "double": ctypes.c_double}


def parse_header(text):
    """(constants, signatures) of a C header written like include/ramp_hip.h: every ``#define RAMP_<NAME> <literal>`` (decimal
    or hex integer, float with an optional f suffix) as name -> value, and every ``ramp_*`` prototype as name -> (restype,
    argtypes).  A parameter with ``*`` or ``[`` is a c_void_p (it takes byref(), arrays, pointer(), c_void_p and None); a
    scalar maps by its type name.  A literal or a type this reader does not know raises: nothing defaults to int."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RAMP_\w+)(.*)$", text, re.M):
        value = value.strip()
        if not value:                               # (the include guard)
            continue
        try:
            constants[name] = int(value, 0)
        except ValueError:
            try:
                constants[name] = float(value[:-1] if value[-1] in "fF" else value)
            except ValueError:
                raise RuntimeError("%s: the value %r is not an integer or float literal" % (name, value)) from None
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{[^{}]*\}[^;]*;", " ", text)
    signatures = {}
    for ret, name, params in re.findall(r"([^;{}()\"]*?)\b(ramp_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, params = " ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")]
        if ret not in _C_RETURNS:
            raise RuntimeError("%s: return type %r is not one this binding maps" % (name, ret))
        argtypes = []
        for p in [] if params == ["void"] else params:
            ctype = " ".join([w for w in p.split() if w != "const"][:-1])       # (the last word is the parameter's name)
            if "*" not in p and "[" not in p and ctype not in _C_SCALARS:
                raise RuntimeError("%s: parameter %r has a type this binding does not map" % (name, p))
            argtypes.append(ctypes.c_void_p if "*" in p or "[" in p else _C_SCALARS[ctype])
        signatures[name] = (_C_RETURNS[ret], argtypes)
    return constants, signatures


def _read_header():
    try:
        with open(HEADER) as f:
            return parse_header(f.read())
    except OSError as e:
        raise RuntimeError("rampvo_amd: cannot read the C header %s (%s): its constants and signatures are taken from it"
                           % (HEADER, e)) from None


# every RAMP_* value macro of the header as a global of this module, under its own name; SIGNATURES: name -> (restype,
# argtypes) of every entry point it declares
CONSTANTS, SIGNATURES = _read_header()
globals().update(CONSTANTS)
KPLANE = 32            # channels per plane of the packed correlation target maps: [h][128 / KPLANE][w][KPLANE]


def kplane(dtype):
    """channels per plane of the packed correlation target maps for a feature dtype: 64 bytes per pixel and plane
    ([h][4][w][32] fp16, [h][8][w][16] fp32).  fp32 features in the split form (corr_f32_mode() == 2) keep the fp32 CONTAINER
    [h][8][w][16] float32 -- the same 512 bytes per pixel -- whose bytes are [h][4][2][w][32] fp16 parts (RAMP_CORR_X2)"""
    import torch
    return KPLANE if dtype == torch.float16 else KPLANE // 2


def corr_f32_mode():
    """how the tracker computes the correlation volume of fp32 features (RAMP_CORR_F32_MFMA, switches.read()): 2 (default)
    split fp16 pairs on the f16 matrix cores (corr_mfma_kernel<CorrX2>, chunked planes of pairs); 1 the fp32 matrix cores
    (corr_mfma_kernel<float>, chunked fp32 planes); 0 corr_kernel<float>, the reference kernel's summation order, plain planes"""
    from . import switches
    return switches.read().corr_f32_mfma

_ERR = {CONSTANTS[name]: "%s (%s)" % (name, why) for name, why in (
    ("RAMP_EINVAL", "bad argument"), ("RAMP_ELAUNCH", "HIP launch/runtime error"),
    ("RAMP_EWORKSPACE", "workspace too small"), ("RAMP_EUNSUPPORTED", "size/shape not supported"))}

c_p, c_i, c_i64, c_sz, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float


class CorrLevel(ctypes.Structure):
    _fields_ = [("fmap", c_p), ("H2", c_i), ("W2", c_i), ("coord_div", c_f)]


def _ptr_fields(names):
    return [(n, c_p) for n in names]


class TrackWeights(ctypes.Structure):
    """ramp_track_weights"""
    _fields_ = (_ptr_fields(["corr_w1", "corr_w2", "corr_w3", "corr_b1", "corr_b2", "corr_b3", "corr_ln_w", "corr_ln_b",
                             "norm_w", "norm_b", "c1_wa", "c1_wb", "c2_wa", "c2_wb", "c1_ba", "c1_bb", "c2_ba", "c2_bb",
                             "kk_wf", "kk_wg", "kk_wh", "ij_wf", "ij_wg", "ij_wh", "kk_bf", "kk_bg", "kk_bh", "ij_bf",
                             "ij_bg", "ij_bh", "ln1_w", "ln1_b", "ln2_w", "ln2_b"])
                + [("gru_w", c_p * 6), ("gru_b", c_p * 6), ("heads_w", c_p), ("heads_b", c_p)]
                + [(n, c_f) for n in ("corr_ln_eps", "norm_eps", "ln1_eps", "ln2_eps")])


class UpdateArgs(ctypes.Structure):
    """ramp_update_args"""
    _fields_ = ([("w", ctypes.POINTER(TrackWeights))]
                + _ptr_fields(["corr", "net_prev", "net_map", "inp", "inp_idx"]) + [("inp_mod", ctypes.c_long), ("state", c_p * 2)]
                + _ptr_fields(["net_out", "relu_out", "coords", "target", "weight", "kk_order", "kk_gid", "kk_seg",
                               "kk_ngroups", "ij_order", "ij_gid", "ij_seg", "ij_ngroups", "ix", "jx", "sagg_frag", "fg",
                               "ykk", "yij", "hkk", "hij"])
                + [(n, c_i) for n in ("kk_cap", "ij_cap", "E", "E_hint", "P", "fp32")] + [("wd", c_f), ("ht", c_f)])


_lib = None


def build(force=False, jobs=8):
    """compile every HIP source for gfx950 into csrc/libramp_hip.so"""
    cmd = ["make", "-s", "-C", CSRC, "-j%d" % jobs]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd + ["libramp_hip.so"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "rampvo_amd: %s is missing -- the HIP extension is not built and there is no "
                "CPU fallback (run __graft_entry__.build())" % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        if l.ramp_corr_kplane() != KPLANE:      # (an older library given through RAMP_HIP_LIB: this binding would pack the planes wrong)
            raise RuntimeError("rampvo_amd: %s packs %d-channel correlation planes, this binding is written for %d "
                               "(the library is older than this binding: rebuild it from csrc/)" % (LIB_PATH, l.ramp_corr_kplane(), KPLANE))
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(rc, "status %d" % rc)))


def stream():
    """the current HIP stream of the current device as a void* (raw getter: this is called ~30x per frame)"""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("rampvo_amd operators run on the GPU only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)


def dtype_code(t):
    if t.dtype == torch.float32:
        return RAMP_F32
    if t.dtype == torch.float16:
        return RAMP_F16
    raise RuntimeError("unsupported dtype %s (float32 / float16 only)" % t.dtype)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_ws_cache = {}
_ws_retired = []
_ws_owner = [None]


class scratch_owner:
    """``with scratch_owner(obj):`` -- scratch taken inside belongs to ``obj`` as well as to the stream.  hipGraph
    captures all run on torch's one capture stream, so the stream alone would hand two captured graphs (two
    Patchifiers, a re-capture) the same scratch buffer although they replay on different streams."""

    def __init__(self, owner):
        self.owner = owner

    def __enter__(self):
        self.prev, _ws_owner[0] = _ws_owner[0], id(self.owner)

    def __exit__(self, *exc):
        _ws_owner[0] = self.prev


def workspace(nbytes, device, tag="ws"):
    """grow-only scratch buffer per (device, stream, owner, tag): two trackers on different streams of one GPU never
    share scratch, and neither do two captured graphs (see ``scratch_owner``).  Contents are never reused across
    calls.  A buffer that is outgrown is retired, not freed: launches already queued on its stream (or captured in
    a hipGraph) may still reference it."""
    key = (device, torch._C._cuda_getCurrentRawStream(device.index if device.index is not None
                                                      else torch.cuda.current_device()), _ws_owner[0], tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def sized_workspace(query, dims, device, tag="ws"):
    """(buffer, nbytes): the scratch buffer of ``workspace`` for an entry point whose size query ``lib().<query>(*dims)``
    returns ``nbytes`` -- the bytes the entry point is told it has (the buffer may be larger)"""
    nbytes = getattr(lib(), query)(*dims)
    return workspace(nbytes, device, tag), nbytes
