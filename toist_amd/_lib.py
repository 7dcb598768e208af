"""ctypes binding of libtoist_hip.so, derived from include/toist_hip.h.

The product path has exactly one backend: the hand-written HIP library.  If it is missing or fails
to load, importing a kernel raises -- there is no CPU or eager-PyTorch fallback.

The header is the only place a signature or a constant is written.  At import this module parses it once
(`parse_signatures`, `parse_constants`: pure functions of the header text) and sets `argtypes` / `restype` of
every `TOIST_API` prototype from what it finds; a parameter it cannot classify raises, it never guesses.  A new
entry point needs its prototype in the header and its launcher in kernels.py, nothing here.  A new descriptor
struct also needs a `Structure` class below (the field names are the launchers' vocabulary; they are not derived)
and its C name in the layout probe's map (tests/test_cpu_host.py: C_STRUCTS), which holds every field of every
class against the C compiler; if the launcher passes it with `byref`, its name goes into `_BYREF` as well.
"""
import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_longlong, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# TOIST_HIP_LIB: another build of the same library (kernel experiments: A/B two builds inside one GPU session)
LIB_PATH = os.environ.get("TOIST_HIP_LIB") or os.path.join(_HERE, "libtoist_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toist_hip.h")

_SCALARS = {"int": c_int32, "int32_t": c_int32, "int64_t": c_int64, "long long": c_longlong, "uint64_t": c_uint64,
            "float": c_float, "size_t": c_size_t}
_INT = r"\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?"


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def parse_constants(text):
    """{name: value} of every `#define TOIST_NAME <integer or (integer)>` and every `TOIST_NAME = <integer>` of an enum body."""
    text = _strip_comments(text)
    out = {name: int(value, 0) for name, value in re.findall(rf"^[ \t]*#[ \t]*define[ \t]+(TOIST_\w+)[ \t]+{_INT}[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", text):
        for entry in filter(None, (e.strip() for e in body.split(","))):
            m = re.fullmatch(rf"(TOIST_\w+)\s*=\s*{_INT}", entry)
            if m is None:
                raise ValueError(f"toist_hip.h: enum entry {entry!r} is not `TOIST_NAME = <integer>`")
            out[m.group(1)] = int(m.group(2), 0)
    return out


def parse_signatures(text, byref):
    """{function: [argtypes]} of every `TOIST_API int toist_name(<params>);` prototype, in the header's order.  A pointer parameter is
    c_char_p (`char*`), POINTER(cls) for the descriptors of `byref` ({C struct name: Structure class}, see _BYREF) and c_void_p
    otherwise (device tables and arrays: the caller casts); a value parameter is one of _SCALARS.  Anything else raises ValueError
    naming the function and the parameter."""
    text = re.sub(r"^[ \t]*#[^\n]*$", "", _strip_comments(text), flags=re.M)         # TOIST_API's own #define lines
    out = {}
    for chunk in re.split(r"\bTOIST_API\b", text)[1:]:
        m = re.match(r"\s+([\w\s*]+?)\s*\b(toist_\w+)\s*\(([^()]*)\)\s*;", chunk)
        if m is None:
            raise ValueError(f"toist_hip.h: TOIST_API is not followed by a prototype: {' '.join(chunk.split())[:80]!r}")
        ret, name, params = m.group(1), m.group(2), [" ".join(p.split()) for p in m.group(3).split(",")]
        if ret != "int" or name in out:
            raise ValueError(f"toist_hip.h: {name}: " + ("declared twice" if ret == "int" else f"returns {ret!r}, every entry point returns int"))
        out[name] = [] if params == ["void"] else [_argtype(name, p, byref) for p in params]
    return out


def _argtype(fn, param, byref):
    *kind, name = [w for w in param.replace("*", " * ").split() if w != "const"] or [""]            # <type> <name>
    stars = kind.count("*")
    base = " ".join(kind[:len(kind) - stars])                                                         # the stars follow the pointee
    if name.isidentifier() and base and "*" not in base:
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 1:
            return c_char_p if base == "char" else POINTER(byref[base]) if base in byref else c_void_p
        if stars > 1:
            return c_void_p                                                                           # a table of pointers
    raise ValueError(f"toist_hip.h: {fn}: cannot bind parameter {param!r}")


try:
    with open(HEADER_PATH) as _f:
        _HEADER = _f.read()
except OSError as e:
    raise RuntimeError(f"{HEADER_PATH} is missing: toist_amd binds libtoist_hip.so from the header it was built against") from e
CONSTANTS = parse_constants(_HEADER)


def _consts(names):
    return [CONSTANTS["TOIST_" + n] for n in names.split()]


TOIST_OK = CONSTANTS["TOIST_OK"]
# operand kinds / activations
A_ROWK, A_KROW, A_CONV, A_CONVT = _consts("A_ROWK A_KROW A_CONV A_CONVT")
B_ROWK, B_KROW, B_CONVX = _consts("B_ROWK B_KROW B_CONVX")
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_MASK_POS, ACT_GELU_BWD, ACT_SIGMOID_BWD = _consts(
    "ACT_NONE ACT_RELU ACT_GELU ACT_SIGMOID ACT_MASK_POS ACT_GELU_BWD ACT_SIGMOID_BWD")
ROW_PLAIN, ROW_LN_FWD, ROW_LN_BWD = _consts("ROW_PLAIN ROW_LN_FWD ROW_LN_BWD")
XDEC_MAX_LAYERS, XDEC_CTL_WORDS = _consts("XDEC_MAX_LAYERS XDEC_CTL_WORDS")
PREP_DESC_WORDS = CONSTANTS["TOIST_PREP_DESC_WORDS"]        # int32 words of one image's row in toist_image_prep's descriptor table
TMASK_DESC_WORDS = CONSTANTS["TOIST_TMASK_DESC_WORDS"]      # int32 words of one slot's row in toist_target_masks' descriptor table
# toist_polygon_masks: int32 words of an object's row and of a polygon's record, the columns of a workgroup's strip, the rows of its LDS plane, the modes
POLY_DESC_WORDS, POLY_REC_WORDS, POLY_STRIP, POLY_MAX_ROWS, POLY_PACKED, POLY_DENSE = _consts(
    "POLY_DESC_WORDS POLY_REC_WORDS POLY_STRIP POLY_MAX_ROWS POLY_PACKED POLY_DENSE")


class Operand(Structure):
    _fields_ = [
        ("ptr", c_void_p), ("bs_outer", c_int64), ("bs_inner", c_int64), ("ld", c_int32), ("kin", c_int32),
        ("tap_stride", c_int64), ("SH", c_int32), ("SW", c_int32), ("SC", c_int32), ("PH", c_int32),
        ("PW", c_int32), ("R", c_int32), ("S", c_int32), ("stride", c_int32), ("pad", c_int32), ("dil", c_int32),
    ]


class Epilogue(Structure):
    _fields_ = [
        ("alpha", c_float), ("scale", c_void_p), ("shift", c_void_p), ("rscale", c_void_p), ("res", c_void_p), ("ldr", c_int32),
        ("aux", c_void_p), ("ldaux", c_int32), ("act", c_int32), ("pre_out", c_void_p), ("out_f32", c_int32),
        ("accumulate", c_int32), ("cmap", c_int32), ("cH", c_int32), ("cW", c_int32), ("cOH", c_int32),
        ("cOW", c_int32), ("cst", c_int32), ("res_div", c_int32), ("res_mod", c_int32), ("drop_where", c_int32), ("drop_p", c_float), ("drop_seed", c_uint64), ("drop_seed_dev", c_void_p),
    ]


class Gemm(Structure):
    _fields_ = [
        ("M", c_int32), ("N", c_int32), ("K", c_int32), ("a_kind", c_int32), ("b_kind", c_int32),
        ("a", Operand), ("b", Operand), ("c", c_void_p), ("ldc", c_int32), ("cs_outer", c_int64),
        ("cs_inner", c_int64), ("batch", c_int32), ("batch_inner", c_int32), ("split_k", c_int32),
        ("tile", c_int32), ("flags", c_int32), ("epi", Epilogue), ("workspace", c_void_p), ("a_colsum", c_void_p),
        ("group", c_void_p), ("a2", c_void_p), ("a2_from", c_int32),
    ]


class RowGemm(Structure):
    """toist_rowgemm_desc (include/toist_hip.h): row-complete sub-layer launch of csrc/tlayer.hip"""
    _fields_ = [
        ("M", c_int32), ("K", c_int32), ("b_kind", c_int32), ("epi", c_int32), ("a", c_void_p), ("w", c_void_p), ("lda", c_int32), ("ldw", c_int32),
        ("fold", c_void_p), ("fold_stride", c_int64), ("fold_parts", c_int32), ("fold_cols", c_int32), ("bias", c_void_p), ("res", c_void_p),
        ("res2", c_void_p), ("ldr", c_int32), ("ldr2", c_int32), ("drop_p", c_float), ("eps", c_float), ("drop_seed", c_uint64),
        ("drop_seed_dev", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("z", c_void_p), ("mean", c_void_p), ("rstd", c_void_p),
        ("out", c_void_p), ("ldo", c_int32), ("reserved", c_int32), ("add", c_void_p), ("out2", c_void_p), ("partials", c_void_p),
    ]


class XdecLayer(Structure):
    """toist_xdec_layer (include/toist_hip.h)"""
    _fields_ = [(n, c_void_p) for n in ("w_in", "b_in", "w_os", "b_os", "g1", "be1", "w_q", "b_q", "w_oc", "b_oc", "g3", "be3", "w1", "b1", "w2", "b2", "g4", "be4")] + \
               [("seed", c_uint64 * 6)]


class Xdec(Structure):
    """toist_xdec_desc (include/toist_hip.h): the XCD-resident decoder stack of csrc/xdec.hip"""
    _fields_ = [("B", c_int32), ("Q", c_int32), ("S", c_int32), ("L", c_int32), ("x0", c_void_p), ("qpos", c_void_p), ("xe0", c_void_p), ("kv", c_void_p), ("ldkv", c_int32),
                ("ff", c_int32), ("test_absent", c_int32), ("reserved", c_int32), ("key_pad", c_void_p), ("drop_p", c_float), ("eps", c_float), ("seed_dev", c_void_p)] + \
               [(n, c_void_p) for n in ("qkv", "ctx_s", "lse_s", "z1", "y1", "y1e", "mean1", "rstd1", "qc", "ctx_c", "lse_c", "z3", "y3", "mean3", "rstd3", "h", "z4", "y4",
                                        "y4e", "mean4", "rstd4", "part", "ctl", "prof")] + \
               [("layer", XdecLayer * XDEC_MAX_LAYERS)]


class XdecBwdLayer(Structure):
    """toist_xdec_bwd_layer (include/toist_hip.h)"""
    _fields_ = [(n, c_void_p) for n in ("w_in", "w_os", "w_q", "w_oc", "w1", "w2", "g1", "g3", "g4")] + [("seed", c_uint64 * 6)]


class XdecBwd(Structure):
    """toist_xdec_bwd_desc (include/toist_hip.h): backward of the XCD-resident decoder stack"""
    _fields_ = [("B", c_int32), ("Q", c_int32), ("S", c_int32), ("L", c_int32), ("kv", c_void_p), ("ldkv", c_int32), ("ldsink", c_int32), ("lddkv", c_int32),
                ("ff", c_int32), ("test_absent", c_int32), ("reserved", c_int32), ("key_pad", c_void_p), ("drop_p", c_float), ("reserved2", c_float), ("seed_dev", c_void_p)] + \
               [(n, c_void_p) for n in ("qkv", "ctx_s", "lse_s", "z1", "mean1", "rstd1", "qc", "ctx_c", "lse_c", "z3", "mean3", "rstd3", "h", "z4", "mean4", "rstd4", "g_out",
                                        "gb4", "dh", "go3", "go1", "sink", "dkv", "ln_part", "dctx", "part", "dq_part", "ctl", "prof")] + \
               [("layer", XdecBwdLayer * XDEC_MAX_LAYERS)]


class ReduceDesc(Structure):
    _fields_ = [("ws", c_void_p), ("out", c_void_p), ("rscale", c_void_p), ("splits", c_int32), ("M", c_int32), ("N", c_int32),
                ("ldc", c_int32), ("alpha", c_float), ("accumulate", c_int32)]


# the descriptors the launchers pass with ctypes.byref: their pointer parameters are typed, every other pointer is a c_void_p
_BYREF = {"toist_gemm": Gemm, "toist_rowgemm_desc": RowGemm, "toist_xdec_desc": Xdec, "toist_xdec_bwd_desc": XdecBwd}
SIGNATURES = parse_signatures(_HEADER, _BYREF)

_lib = None


def exported_symbols():
    """Names every include/toist_hip.h entry point must be exported under."""
    return sorted(SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        # torch ships its own HIP runtime (libamdhip64); it must be the one already loaded when our
        # library binds, otherwise two runtimes coexist and launches fail with "no ROCm-capable device".
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(toist_amd has no CPU / eager fallback)"
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        _lib = handle
    return _lib


def last_error():
    buf = ctypes.create_string_buffer(512)
    lib().toist_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc, what):
    if rc != TOIST_OK:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")
