"""Wave primitives live in one header (csrc/dq_wave.h), and the LinearAttention backward's retired build-time
experiments stay retired.  Reads the sources; no GPU, no build."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-deconvolution-dia-msms-data_amd")
CSRC = os.path.join(PKG, "csrc")
HEADER = "dq_wave.h"


def _sources():
    return {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".cpp", ".h"))}


def _files_with(pattern):
    return [n for n, text in _sources().items() if re.search(pattern, text)]


def test_fp32_mfma_builtins_only_in_the_shared_header():
    for builtin in ("__builtin_amdgcn_mfma_f32_4x4x1f32", "__builtin_amdgcn_mfma_f32_16x16x4f32", "__builtin_amdgcn_mfma_f32_32x32x2f32"):
        assert _files_with(re.escape(builtin)) == [HEADER], builtin


def test_float4_vector_typedef_only_in_the_shared_header():
    assert _files_with(r"typedef\s+float\s+\w+\s+__attribute__\(\(ext_vector_type\(4\)\)\)") == [HEADER]


def test_retired_la_bwd_experiments_are_gone():
    texts = _sources()
    texts["Makefile"] = open(os.path.join(PKG, "Makefile")).read()
    for name in ("DQ_LA_PF4", "DQ_LA_12TW", "DQ_LA_4_3W", "DQ_LA_BIG_TU"):
        assert [n for n, text in texts.items() if name in text] == [], name
