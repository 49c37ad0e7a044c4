"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads without a GPU and exports every
symbol include/madtp_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from madtp_amd import build
    return build.build(verbose=False)


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "madtp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    syms = _header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/madtp_hip.h but not exported"


def test_binding_matches_header(lib_path):
    from madtp_amd import hip
    assert hip.exported_symbols() == _header_symbols()
    lib = hip.load()
    assert lib.madtp_abi_version() == hip.ABI_VERSION
    assert lib.madtp_strerror(-2) == b"unsupported shape"


STRUCT_SIZES = {"madtp_att_ft_seg": 40, "madtp_lin": 32, "madtp_vit_block_w": 200, "madtp_bert_layer_w": 528, "madtp_query_w": 56,
                "madtp_layer_io": 96}


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof / offsetof of the six structs from the compiler the library is built with (host only) against the ctypes classes the
    binding derives from the header; the program's field list comes from the Python classes, so a field missing on either side
    fails the compile or the compare."""
    import subprocess
    from madtp_amd import abi, build, hip
    classes = {"madtp_lin": hip.LinStruct, "madtp_vit_block_w": hip.VitBlockW, "madtp_bert_layer_w": hip.BertLayerW,
               "madtp_query_w": hip.QueryW, "madtp_layer_io": hip.LayerIO, "madtp_att_ft_seg": hip.AttFtSeg}
    assert classes == abi.STRUCTS and set(classes) == set(STRUCT_SIZES)
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "madtp_hip.h"', "int main() {"]
    for cname, cls in classes.items():
        lines.append(f'    std::printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    std::printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([build._hipcc(), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {}
    for cname, cls in classes.items():
        want[cname] = str(ctypes.sizeof(cls))
        want.update({f"{cname}.{f[0]}": str(getattr(cls, f[0]).offset) for f in cls._fields_})
        assert ctypes.sizeof(cls) == STRUCT_SIZES[cname]
    assert got == want
    # every field the header declares is a field of the class (the compare above walks the class's fields only)
    text = re.sub(r"/\*.*?\*/", "", open(abi.HEADER).read(), flags=re.S)
    for cname, cls in classes.items():
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}" % cname, text, flags=re.S).group(1)
        declared = [d.split("[")[0].split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for d in decl.split(",")]
        assert declared == [f[0] for f in cls._fields_]


def test_signatures_come_from_the_header(lib_path):
    from ctypes import c_float, c_int, c_size_t, c_uint64, c_void_p
    from madtp_amd import abi, hip
    sigs = abi.SIGNATURES
    assert sigs["madtp_gemm"] == (c_int, [c_void_p] * 5 + [c_int] * 10 + [c_float, c_float, c_void_p])
    assert sigs["madtp_attention_bwd"] == (
        c_int, [c_void_p] * 3 + [c_int] + [c_void_p] * 2 + [c_int, c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 6
        + [c_int, c_void_p, c_size_t, c_void_p] + [c_int] * 3 + [c_float, c_float, c_uint64, c_uint64, c_void_p])
    assert sigs["madtp_bert_layer"] == (
        c_int, [c_void_p] * 7 + [c_size_t] + [c_int] * 3 + [c_void_p] + [c_int] * 3 + [c_float] + [c_void_p] * 5 + [c_int]
        + [c_void_p] * 9 + [c_int] + [c_void_p] * 3)
    assert sigs["madtp_strerror"] == (ctypes.c_char_p, [c_int]) and sigs["madtp_profile_end"] == (c_int, [ctypes.c_char_p, c_int])
    assert sigs["madtp_abi_version"] == (c_int, []) and sigs["madtp_vit_block_workspace"] == (c_size_t, [c_int] * 6)
    assert len(sigs) == len(_header_symbols()) == 97
    lib = hip.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is res, name


@pytest.mark.parametrize("text", [
    "int madtp_bad(long double x, void* stream);",                                   # a type outside the mapping rule
    "int madtp_bad(void (*callback)(int), void* stream);",                           # a function-pointer argument
    "typedef struct madtp_bad_w { madtp_missing lin; int n; } madtp_bad_w;",         # a field of an undeclared type
    "int madtp_bad(int);",                                                           # no declarator to split
    "typedef struct madtp_bad_w { int (*f)(void); } madtp_bad_w;",
], ids=["long_double", "function_pointer", "undeclared_field_type", "unnamed_argument", "function_pointer_field"])
def test_parser_refuses_what_it_does_not_know(text):
    from madtp_amd import abi
    good = "#define MADTP_X (-3)\ntypedef struct madtp_p { const float *a, *b; int n[2]; } madtp_p;\nint madtp_ok(const madtp_p* p, size_t n);\n"
    sigs, structs, defines = abi.parse(good)
    assert sigs == {"madtp_ok": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t])} and defines == {"MADTP_X": -3}
    assert [f[0] for f in structs["madtp_p"]._fields_] == ["a", "b", "n"] and ctypes.sizeof(structs["madtp_p"]) == 24
    with pytest.raises(ValueError, match="madtp_hip.h"):
        abi.parse(good + text)


def test_constants_come_from_the_header(lib_path):
    from madtp_amd import abi, hip
    assert hip.F16S == 2 and hip.E_RANGE == -6 and hip.ATTN_PLAN_PAIR_MASKS_DIFFER == 16384
    assert hip.ABI_VERSION == hip.load().madtp_abi_version() == 31
    assert (hip.F32, hip.BF16, hip.F16) == (0, 1, 3) and (hip.ACT_NONE, hip.ACT_GELU, hip.ACT_QUICK_GELU, hip.ACT_RELU) == (0, 1, 2, 3)
    assert (hip.PLAN_PAIR, hip.PLAN_BIAS, hip.PLAN_RESIDUAL, hip.PLAN_M_DEV) == (1, 2, 4, 8) and (hip.ATTN_RES_HM, hip.ATTN_RES_OPART) == (1, 2)
    assert len(hip.PLAN_FIELDS) == abi.DEFINES["MADTP_PLAN_FIELDS"] and len(hip.ATTN_PLAN_FIELDS) == abi.DEFINES["MADTP_ATTN_PLAN_FIELDS"]


def test_prune_record():
    from madtp_amd import hip
    keys = ["k", "score", "threshold", "count", "pruned", "indices", "indices_sort"]
    a, b = hip.prune_info(3, "s", "t", "c"), hip.prune_info(3, "s", "t", "c", "i", "o")
    assert list(a) == keys == list(b) and a["pruned"] is False and a["indices"] is None and a["indices_sort"] is None
    assert b["pruned"] is True and (b["k"], b["score"], b["threshold"], b["count"], b["indices"], b["indices_sort"]) == (3, "s", "t", "c", "i", "o")
    lazy = hip.LazyPruneInfo(lambda: b)
    assert dict(lazy.items()) == b


def test_argument_validation_without_gpu(lib_path):
    # argument checks run on the host before any launch: usable as a no-GPU smoke of the error contract
    from madtp_amd import hip
    lib = hip.load()
    assert lib.madtp_gemm(0, 0, 0, 0, 0, 1, 1, 64, 64, 64, 1, 0, 1, 1, 0, 1.0, 1.0, 0) == -1      # null pointers
    assert lib.madtp_gemm(16, 16, 0, 0, 16, 4, 4, 40, 40, 40, 4, 0, 1, 1, 0, 1.0, 1.0, 0) == -2   # K*2 % 128 != 0
    assert lib.madtp_gemm(16, 16, 0, 0, 16, 4, 4, 64, 64, 64, 4, 0, 7, 1, 0, 1.0, 1.0, 0) == -3   # dtype
    assert lib.madtp_gemm(8, 16, 0, 0, 16, 4, 4, 64, 64, 64, 4, 0, 1, 1, 0, 1.0, 1.0, 0) == -4    # alignment
    assert lib.madtp_token_select(16, 0, 16, 16, 16, 16, 2, 8, 0) == -2                       # k < 1


def test_product_path_refuses_cpu_tensors(lib_path):
    import torch
    from madtp_amd import hip
    with pytest.raises(RuntimeError):
        hip.gemm(torch.zeros(4, 64), torch.zeros(128, 64))
