"""CPU: the C-ABI library exists, loads, and exports every symbol include/c2m_hip.h declares, and the ctypes mirror of
c2m_amd/_lib.py (prototypes and descriptor structs) agrees with that header (no compute calls)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/c2m_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "c2m_hip.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(c2m_[a-z0-9_]+)\s*\(", _header())))


_SCALARS = ("int", "float", "double", "long long", "size_t")


def _param_kind(decl):
    """'const float* x' -> 'pointer', 'long long nblocks' -> 'long long': the C type of one parameter, as the ABI passes it"""
    if "*" in decl or "c2m_stream_t" in decl:
        return "pointer"
    kind = " ".join(decl.replace("const", " ").split()[:-1])   # drop the parameter's name
    assert kind in _SCALARS, decl
    return kind


def _prototypes():
    """{name: (return kind, [parameter kinds])} of every c2m_* function the header declares"""
    protos = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \*]*?)\s*\b(c2m_\w+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M):
        params = " ".join(params.split())
        protos[name] = (_param_kind(ret + " _"), [] if params == "void" else [_param_kind(d) for d in params.split(",")])
    return protos


def _ctypes_kind(t):
    scalar = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_longlong: "long long",
              ctypes.c_size_t: "size_t"}
    if t in scalar:
        return scalar[t]
    assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), t
    return "pointer"


def test_header_declares_the_expected_entry_points():
    names = _declared()
    for must in ("c2m_feature_match_index_f32", "c2m_feature_normalize_f32", "c2m_build_pre_offsets_f32",
                 "c2m_dcn_v2_forward_f32", "c2m_dcn_v2_forward_bf16mma_f32", "c2m_dcn_v2_backward_f32", "c2m_dcn_fuse_offsets_f32", "c2m_abi_version"):
        assert must in names


def test_library_exports_every_declared_symbol_at_abi_6():
    import c2m_amd
    assert os.path.exists(c2m_amd.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(c2m_amd.LIB_PATH)
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.c2m_abi_version() == 6
    lib.c2m_status_string.restype = ctypes.c_char_p
    assert lib.c2m_status_string(0) == b"ok" and b"workspace" in lib.c2m_status_string(3)


def test_ctypes_prototypes_match_the_header():
    """Arity and every scalar kind of the argtypes _lib._declare sets are the header's: a miscounted list or an int where the
    header says long long would not raise, it would shift every later argument."""
    import c2m_amd
    L = c2m_amd._lib.lib()
    protos = _prototypes()
    assert sorted(protos) == _declared() and len(protos) == 56
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert _ctypes_kind(fn.restype) == ret, name
        if params:
            assert fn.argtypes is not None, f"{name}: _lib._declare sets no argtypes"
            assert [_ctypes_kind(t) for t in fn.argtypes] == params, name
        else:
            assert not fn.argtypes, name


_STRUCTS = {"c2m_conv_src": "ConvSrc", "c2m_conv3x3_desc": "Conv3x3Desc", "c2m_image_src": "ImageSrc",
            "c2m_conv3x3_rgb64_desc": "Conv3x3Rgb64Desc", "c2m_dcn_nhwc_desc": "DcnNhwcDesc"}


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """sizeof and every offsetof of the descriptor structs, printed by a C program that includes the header, against the
    ctypes.Structure mirrors (host compiler only, nothing runs on a GPU)."""
    import c2m_amd
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.skip("no C compiler on this machine")
    hdr = _header()
    assert sorted(re.findall(r"typedef struct (c2m_\w+)", hdr)) == sorted(_STRUCTS)
    lines, want = [], []
    for cname, pyname in _STRUCTS.items():
        cls = getattr(c2m_amd._lib, pyname)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        names = [re.search(r"(\w+)\s*(\[\d+\])?$", f.strip()).group(1) for decl in body.split(";") if decl.strip() for f in decl.split(",")]
        assert names == [n for n, _ in cls._fields_], cname
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(cls))
        for n in names:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, n))
            want.append(getattr(cls, n).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2m_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want and len(want) >= 47 + 2


def test_product_path_never_touches_the_oracle():
    pkg = os.path.join(REPO, "c2-matching_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(root, f)).read()
                assert "c2m_oracle" not in src and "torch_port" not in src and "oracle/" not in src.replace("the oracle", ""), os.path.join(root, f)


def test_cpu_tensors_are_rejected_not_emulated():
    import pytest
    import torch
    import c2m_amd
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.feature_match_index_batched(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.dcn_v2_forward(torch.zeros(1, 4, 5, 5), torch.zeros(2, 4, 3, 3), torch.zeros(2), torch.zeros(1, 18, 5, 5), torch.zeros(1, 9, 5, 5))


def test_correlation_workspace_is_sized_by_the_maps_channels():
    """the pre-filter's per-channel scratch follows C (none where the filter has no kernel); the C-less query keeps
    returning the 256-channel upper bound, which every layout fits (no GPU needed: pure size arithmetic in the library)."""
    import c2m_amd
    L = c2m_amd._lib.lib()
    shp = (16, 160, 160, 160, 160)
    upper = L.c2m_feature_match_workspace_bytes(*shp)
    by_c = {c: L.c2m_feature_match_workspace_bytes_c(shp[0], c, *shp[1:]) for c in (32, 64, 128, 256)}
    assert by_c[256] == upper and by_c[64] < by_c[128] < by_c[256]
    assert by_c[32] < 64 << 20 < by_c[64]                 # no filter kernel for C = 32: tables only
    per_c = (by_c[256] - by_c[128]) / 128                 # bytes per channel of the four per-channel blocks
    assert abs((by_c[128] - by_c[64]) / 64 - per_c) <= 1024 and abs(by_c[64] - by_c[32] - 64 * per_c) <= 4096
    assert L.c2m_feature_match_workspace_bytes_c(0, 256, 160, 160, 160, 160) == 0
