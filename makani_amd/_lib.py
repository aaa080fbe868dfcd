"""ctypes binding of libmakani_amd.so, derived from the C ABI in include/makani_amd.h.

The header is parsed once, at import: its ``#define MK_*`` integer constants (``CONSTS``), its descriptor structs as
``ctypes.Structure`` classes (``STRUCTS``) and every prototype as ``(argtypes, restype)`` (``_SIGS``).  Nothing of the
interface is written down here a second time: a new entry point is its prototype in the header and its definition in
``csrc``.  A declaration the parser does not understand raises at import, naming the line.

The product path has no CPU fallback: if the shared library is missing or a
tensor is not on a GPU, calls raise.  Build with ``python -m makani_amd.build``.
"""
import ast
import ctypes as C
import operator
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "makani_amd.h")          # the C ABI: the binding below and build.py's dependency check
# MAKANI_AMD_LIB: a variant of the library built by tools/ab.py (same-box A/B measurements); default: the in-tree build
LIB_PATH = os.environ.get("MAKANI_AMD_LIB") or os.path.join(_HERE, "libmakani_amd.so")

c_vp = C.c_void_p

_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double}
_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul}


def _const_expr(expr, names):
    """value of an integer constant expression: literals, the names known so far, + - * and parentheses, nothing else"""
    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.Name) and n.id in names:
            return names[n.id]
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, (ast.USub, ast.UAdd)):
            return -ev(n.operand) if isinstance(n.op, ast.USub) else ev(n.operand)
        if isinstance(n, ast.BinOp) and type(n.op) in _OPS:
            return _OPS[type(n.op)](ev(n.left), ev(n.right))
        raise ValueError(f"{expr.strip()!r} is not an integer constant expression"
                         + (f" (unknown name {n.id})" if isinstance(n, ast.Name) else ""))
    try:
        return ev(ast.parse(expr.strip(), mode="eval").body)
    except SyntaxError:
        raise ValueError(f"{expr.strip()!r} is not an integer constant expression") from None


def _ctype(spec, structs, ret=False):
    """the ctypes type of a type as the header spells it ("long long", "const float*", "const MkGemm*")"""
    words = [w for w in spec.replace("*", " * ").split() if w != "const"]
    base, stars = " ".join(w for w in words if w != "*"), words.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars == 1 and (base in _SCALARS or base == "void"):
        return C.c_void_p
    if ret and (base, stars) in (("char", 1), ("void", 0)):
        return C.c_char_p if stars else None
    raise ValueError(f"type {' '.join(spec.split())!r} is outside the vocabulary of the header")


def parse_header(text, name="makani_amd.h"):
    """(constants, structs, prototypes) of the header ``text``: {MK_NAME: int}, {struct name: ctypes.Structure class},
    {function: (argtypes, restype)}.  Raises ValueError naming the line of whatever it does not understand."""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group())          # positions and line numbers stay those of the file

    def fail(pos, msg):
        return ValueError(f"{name}:{text.count(chr(10), 0, pos) + 1}: {msg}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    consts, structs, protos = {}, {}, {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(MK_\w+)[ \t]+(\S.*)$", text, re.M):
        try:
            consts[m.group(1)] = _const_expr(m.group(2), consts)
        except ValueError as e:
            raise fail(m.start(), f"{m.group(1)}: {e}") from None
    text = re.sub(r"^[ \t]*#ifdef __cplusplus.*?^[ \t]*#endif", blank, text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#.*$", blank, text, flags=re.M)
    ndecl = len(re.findall(r"\bmk_\w*\s*\(", text))

    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        fields, pos = [], m.start(2)
        for decl in m.group(2).split(";")[:-1]:
            first, *more = decl.split(",")
            d = re.fullmatch(r"\s*(.*?)(\w+)\s*((?:\[[^\]]*\]\s*)*)", first, re.S)
            try:
                if not d or any("*" in x for x in more):
                    raise ValueError(f"cannot read the field declaration {' '.join(decl.split())!r}")
                base = C.c_void_p if "*" in d.group(1) else _ctype(d.group(1), {})
                for x in [d.group(2) + d.group(3)] + more:
                    fname, t = re.match(r"\s*(\w*)", x).group(1), base
                    if not re.fullmatch(r"\s*\w+\s*(\[[^\]]*\]\s*)*", x):
                        raise ValueError(f"cannot read the declarator {x.strip()!r}")
                    for extent in reversed(re.findall(r"\[([^\]]*)\]", x)):
                        t = t * _const_expr(extent, consts)
                    fields.append((fname, t))
            except ValueError as e:
                raise fail(pos + len(decl) - len(decl.lstrip()), f"struct {m.group(1)}: {e}") from None
            pos += len(decl) + 1
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields, "__doc__": f"`struct {m.group(1)}` of {name}"})
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{.*?\}\s*\1\s*;", blank, text, flags=re.S)

    pos = 0
    for stmt in text.split(";"):
        at, pos = pos + len(stmt) - len(stmt.lstrip()), pos + len(stmt) + 1
        if not stmt.strip():
            continue
        m = re.fullmatch(r"\s*([^()]+?)\b(mk_\w*)\s*\(([^()]*)\)\s*", stmt, re.S)
        if not m:
            raise fail(at, f"not a prototype: {' '.join(stmt.split())[:80]!r}")
        try:
            params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
            args = []
            for p in params:
                d = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, re.S)
                if not d or not d.group(1).strip():
                    raise ValueError(f"cannot read the parameter {' '.join(p.split())!r}")
                args.append(_ctype(d.group(1), structs))
            protos[m.group(2)] = (args, _ctype(m.group(1), structs, ret=True))
        except ValueError as e:
            raise fail(at, f"{m.group(2)}: {e}") from None
    if len(protos) != ndecl:
        raise ValueError(f"{name}: understood {len(protos)} prototypes, but the header declares {ndecl} mk_...( entry points")
    return consts, structs, protos


with open(HEADER) as _f:
    CONSTS, STRUCTS, _SIGS = parse_header(_f.read())

MK_F32, MK_BF16, MK_FFT_SEG_MAX = (CONSTS[k] for k in ("MK_F32", "MK_BF16", "MK_FFT_SEG_MAX"))
TRI_NONE, TRI_ROW_GE, TRI_K_GE, TRI_ROW_LE, TRI_K_LE = (CONSTS["MK_TRI_" + k] for k in ("NONE", "ROW_GE", "K_GE", "ROW_LE", "K_LE"))
MkGemm, MkFftSeg, MkAdamTensor = (STRUCTS[k] for k in ("MkGemm", "MkFftSeg", "MkAdamTensor"))
EXPORTS = sorted(_SIGS)

_lib = None


def lib():
    """Load (once) and return the shared library; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MI355X HIP library has not been built "
                "(run `python -m makani_amd.build`).  There is no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().mk_last_error().decode()
        raise RuntimeError(f"libmakani_amd {what} failed (code {rc}): {msg}")


def stream():
    return c_vp(torch.cuda.current_stream().cuda_stream)


def device_guard(fn):
    """Module ``forward``s of the package run with the CURRENT device = the device of their first tensor argument: every
    C-ABI launch goes to ``torch.cuda.current_stream()`` of the current device, so a model living on cuda:1 while the
    process's current device is cuda:0 would otherwise enqueue its kernels on the wrong device's stream.  (Backward nodes
    run on autograd's per-device worker threads, which set the device themselves.)"""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        # the first CUDA tensor among the positional, then the keyword arguments decides (model(x=inp), loss(prd=, tar=))
        for a in (*args, *kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(self, *args, **kwargs)
                break
        return fn(self, *args, **kwargs)

    return wrapped


def ptr(t):
    if t is None:
        return c_vp(0)
    if not t.is_cuda:
        raise RuntimeError("makani_amd ops need GPU tensors (the HIP path has no CPU fallback)")
    return c_vp(t.data_ptr())


def need_gpu(t, what="losses"):
    if not t.is_cuda:
        raise RuntimeError(f"makani_amd {what} run on the GPU (HIP) path only")


def prep(t, ref_shape=None):
    """``t`` as a contiguous f32 | bf16 tensor (other dtypes: cast to f32), expanded to ``ref_shape`` when that is given"""
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    if ref_shape is not None and tuple(t.shape) != tuple(ref_shape):
        t = t.expand(ref_shape)
    return t.contiguous()


def dtype_code(t):
    if t.dtype == torch.float32:
        return MK_F32
    if t.dtype == torch.bfloat16:
        return MK_BF16
    raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def dense_view(t):
    """``t`` as a contiguous view in MEMORY order (its dims permuted by decreasing stride), or None when ``t`` has gaps or
    overlaps.  Element-wise kernels (optimizer, norms, all-reduce) run on this view of tensors that are dense but not
    C-contiguous — the native-order dhconv weight, its gradient and its optimizer state."""
    if t.is_contiguous():
        return t
    order = sorted(range(t.dim()), key=lambda d: (-t.stride(d), -t.size(d)))
    v = t.permute(order)
    return v if v.is_contiguous() else None
