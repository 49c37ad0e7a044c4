"""The C ABI of libmadtp_hip.so as include/madtp_hip.h declares it: the header is the ONE declaration, read here once per process.

    SIGNATURES  name -> (restype, [argtypes])     every `madtp_*(...)` prototype
    STRUCTS     C name -> ctypes.Structure class  every `typedef struct`, fields in the header's order
    DEFINES     name -> int                       every integer `#define MADTP_*`

The mapping rule: any pointer is c_void_p, except `char*` / `const char*` = c_char_p; int, float, double, size_t, int32_t, int64_t,
uint32_t and uint64_t are the ctypes type of the same name (`unsigned long long` = c_uint64); `(void)` is an empty argument list.
This is not a C parser: it takes what this header uses and refuses (ValueError naming the text) anything else - an unknown type, a
declarator it cannot split, a `madtp_*(` without a signature - because a guessed argument type fails on the GPU, not at import.

The side headers next to it (madtp_image.h, madtp_augment.h, madtp_jpeg.h, madtp_jhuff.h, madtp_search.h, madtp_csearch.h, madtp_lists.h) are read the same way by
bind(), which also returns the lib() that sets their signatures on the loaded library and checks their own version number."""
import ctypes
import os
import re
import threading

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "madtp_hip.h")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "unsigned long long": ctypes.c_uint64}
_NAME = r"[A-Za-z_]\w*"
_DECLARATOR = rf"((?:\*\s*)*)({_NAME})\s*(?:\[(\d+)\])?\s*"  # stars, name, array length: `*ln1_b`, `cq[2]`


def _ctype(base, stars, structs, where, header):
    base = " ".join(base.split())
    if stars:
        return ctypes.c_char_p if (base, stars) == ("char", 1) else ctypes.c_void_p
    if base in _SCALARS:
        return _SCALARS[base]
    if base in structs:
        return structs[base]
    raise ValueError(f"{header}: unknown type {base!r} in {where.strip()!r}")


def _declaration(text, structs, header):
    """`const float *g, *b` / `madtp_lin cq[2], merge` -> [(name, ctype)]: the star and the array length belong to the declarator"""
    first, *rest = re.sub(r"\bconst\b", " ", text).split(",")
    m = re.fullmatch(rf"\s*({_NAME}(?:\s+{_NAME})*?)(?=[\s*])\s*{_DECLARATOR}", first)
    more = [re.fullmatch(rf"\s*{_DECLARATOR}", d) for d in rest]
    if m is None or None in more:
        raise ValueError(f"{header}: cannot split the declaration {text.strip()!r}")
    out = []
    for stars, name, count in [m.groups()[1:]] + [d.groups() for d in more]:
        t = _ctype(m.group(1), stars.count("*"), structs, text, header)
        out.append((name, t * int(count) if count else t))
    return out


def parse(text, header="madtp_hip.h"):
    """header text -> (signatures, structs, defines), see the module docstring; `header` is the file's name in every ValueError"""
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MADTP_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", src, flags=re.M)}
    src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)
    structs = {}
    for body, cname in re.findall(rf"typedef\s+struct\s+{_NAME}\s*\{{(.*?)\}}\s*({_NAME})\s*;", src, flags=re.S):
        fields = [f for decl in body.split(";") if decl.strip() for f in _declaration(decl, structs, header)]
        structs[cname] = type(cname, (ctypes.Structure,), {"_fields_": fields})
    src = re.sub(r"typedef\s+struct\b.*?\}\s*\w+\s*;", "", src, flags=re.S)
    sigs = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(madtp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ret = re.sub(r"\bconst\b", " ", ret)
        if "[" in args:
            raise ValueError(f"{header}: array argument in {name}({args.strip()})")
        argtypes = [] if args.strip() == "void" else [t for a in args.split(",") for _, t in _declaration(a, {}, header)]
        sigs[name] = (_ctype(ret.replace("*", " "), ret.count("*"), {}, ret + name, header), argtypes)
    lost = sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)) - set(sigs))
    if lost:
        raise ValueError(f"{header}: no signature could be read for {', '.join(lost)}")
    return sigs, structs, defines


def _read(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise RuntimeError(f"{path} not readable ({e}): the binding takes every signature, struct and constant from it") from e


SIGNATURES, STRUCTS, DEFINES = parse(_read(HEADER))


# ---- the side headers (madtp_image.h, madtp_jpeg.h, ...): each has its own version number and is bound on first use ---------------
_bind_lock = threading.Lock()


def binder(signatures, defines, version_symbol, needs=None):
    """-> lib(): hip.load()'s handle with `signatures` set on it and the library's `version_symbol`() checked against the header's
    define of the same name in capitals.  Both happen once, under a lock: lib() may be first called from a decoder's worker threads.
    needs: the lib() of the module whose entry points this one also calls, bound first."""
    family = version_symbol[len("madtp_"):-len("_abi_version")]
    want = defines[version_symbol.upper()]
    bound = []

    def lib():
        if bound:
            return bound[0]
        from . import hip
        h = hip.load() if needs is None else needs()
        with _bind_lock:
            if not bound:
                for name, (res, args) in signatures.items():
                    fn = getattr(h, name)  # AttributeError => header/library mismatch
                    fn.restype = res
                    fn.argtypes = args
                got = getattr(h, version_symbol)()
                if got != want:
                    raise RuntimeError(f"libmadtp_hip {family} ABI {got} != binding {want}; rebuild")
                bound.append(h)
        return h

    return lib


def bind(header_file, version_symbol, prefix=None, needs=None):
    """A header next to madtp_hip.h -> (SIGNATURES, DEFINES, lib): what parse() reads from it - of the signatures only those that
    begin with `prefix`, where one is given (a header that includes another declares its own family) - and their binder()."""
    signatures, _, defines = parse(_read(os.path.join(os.path.dirname(HEADER), header_file)), header_file)
    if prefix is not None:
        signatures = {k: v for k, v in signatures.items() if k.startswith(prefix)}
    return signatures, defines, binder(signatures, defines, version_symbol, needs)
