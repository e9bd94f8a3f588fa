"""The ctypes bindings _lib.py derives from include/reidmi.h: the parser's output pinned for
declarations that between them use every mapping rule, what the parser refuses, and the derived
struct layouts against the compiler's own sizeof / offsetof.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

VP, I32, I64, F32, F64, U16 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double,
                               ctypes.c_uint16)
# C struct -> the name model.py exports it under
STRUCTS = {"reidmi_block_weights": "BlockWeights", "reidmi_vit_weights": "VitWeights",
           "reidmi_text_weights": "TextWeights", "reidmi_block_src": "BlockSrc", "reidmi_vit_src": "VitSrc",
           "reidmi_text_src": "TextSrc", "reidmi_conv_weights": "ConvWeights",
           "reidmi_bottleneck_weights": "BottleneckWeights", "reidmi_resnet_weights": "ResnetWeights",
           "reidmi_convbn_src": "ConvBnSrc", "reidmi_bottleneck_src": "BottleneckSrc",
           "reidmi_resnet_src": "ResnetSrc"}


def test_pinned_declarations():
    from multimodal_reid_amd import _lib, model
    d = _lib.declarations(tools=True)
    assert d["reidmi_rerank"] == (I32, [VP, I64, I64, I64, I64, I32, I32, U16, F32, VP, I64, VP, I64, VP, VP])
    assert d["reidmi_prof_collect_min"] == (I32, [I32, F64, VP, VP, VP])
    assert d["reidmi_rr_rank_rows_f16_pass_rows"] == (I64, [I64, I64, I64, I32, I32])
    assert d["reidmi_rr_jaccard_topk_rows"] == (I32, [VP, I64, I64, I64, VP, VP, I64, I64, I64, VP, VP, VP, VP, VP,
                                                      VP, U16, F32, I32, VP, VP, VP, VP, VP, VP, I64, VP, I64, VP,
                                                      I64, VP, I64, VP])
    assert d["reidmi_comm_init"] == (I32, [VP, I32, I32, VP, I32])
    assert d["reidmi_comm_destroy"] == (I32, [VP])
    assert d["reidmi_resnet_forward"] == (I32, [ctypes.POINTER(model.ResnetWeights), VP, I32, I64, I32, I32, VP, I32,
                                                VP, VP, VP, VP, VP, I64, VP])
    assert d["reidmi_last_error"] == (ctypes.c_char_p, [])
    assert d["reidmi_files_size"] == (I32, [VP, I64, VP, I32])  # const char* const*
    assert d["reidmi_search_ex_workspace_bytes"] == (I64, [I64, I64, I64, I32, I32, I32])  # reidmi_tools.h
    assert "reidmi_search_ex_workspace_bytes" not in _lib.declarations()


def test_model_exports_the_derived_structs():
    from multimodal_reid_amd import _lib, model
    derived = _lib.structs()
    assert set(derived) == set(STRUCTS)
    for cname, name in STRUCTS.items():
        assert getattr(model, name) is derived[cname]
    fields = dict(model.ResnetWeights._fields_)
    assert fields["layers"] is I32 * 4 and fields["stem"] is model.ConvWeights * 3 and fields["tta_pad"] is F32 * 3
    assert fields["blocks"] is ctypes.POINTER(model.BottleneckWeights) and fields["pos_emb"] is VP
    assert dict(model.BottleneckWeights._fields_)["down"] is model.ConvWeights


@pytest.mark.parametrize("header,message", [
    ("int reidmi_f(const float* x, size_t n);", "unknown type `size_t`"),
    ("int reidmi_f(struct other* x);", "unknown type"),
    ("void reidmi_f(int n);", "unknown result type `void`"),
    ("typedef struct reidmi_s { int32_t a; long b; } reidmi_s;", "unknown type `long` in `reidmi_s: long b`"),
    ("typedef struct reidmi_s { const float* a, b; } reidmi_s;", "cannot parse field"),
    ("typedef struct reidmi_s { int32_t a; } reidmi_t;", "is named reidmi_t"),
    ("int reidmi_f(int (*callback)(int));", "cannot parse declaration"),
    ("int reidmi_f(int64_t, int n);", "cannot parse argument `int64_t`"),
    ("int reidmi_f(int n, ...);", "cannot parse argument `...`"),
    ("int reidmi_f(int n) { return n; }", "cannot parse declaration"),
    ("struct reidmi_s { int a; };", "cannot parse declaration"),
    ("int other_f(int n);", "cannot parse declaration `int other_f(int n)`"),
])
def test_parser_refuses_what_it_does_not_know(header, message):
    from multimodal_reid_amd import _lib
    assert _lib.parse_header("int reidmi_f(const float* x, int n);")[1] == {"reidmi_f": (I32, [VP, I32])}
    with pytest.raises(_lib.ReidmiError) as e:
        _lib.parse_header("/* c */ int reidmi_ok(void); // c\n#define X 1\n" + header)
    assert message in str(e.value), str(e.value)


def _header_fields():
    """{struct: [field names]} by this file's own regex (not the parser under test)."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "reidmi.h")).read(), flags=re.S)
    return {name: re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
            for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}", txt, flags=re.S)}


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every field's offsetof / size as the C++ compiler lays reidmi.h out, against
    ctypes.sizeof and Cls.<field>.offset / .size of the classes derived from the header."""
    from multimodal_reid_amd import _lib, build_lib
    if not shutil.which(build_lib.HIPCC):
        pytest.skip("hipcc not available")
    fields = _header_fields()
    assert set(fields) == set(STRUCTS)
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "reidmi.h"', "int main() {"]
    for s, names in fields.items():
        lines.append(f'  std::printf("{s} - %zu 0\\n", sizeof({s}));')
        lines += [f'  std::printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in names]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([build_lib.HIPCC, "-x", "c++", "-std=c++17", f"-I{build_lib.INCLUDE}", str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    compiler = [tuple(l.split()) for l in out if l]
    derived = []
    for s in fields:
        cls = _lib.structs()[s]
        derived.append((s, "-", str(ctypes.sizeof(cls)), "0"))
        derived += [(s, f, str(getattr(cls, f).offset), str(getattr(cls, f).size)) for f, _ in cls._fields_]
    assert derived == compiler
