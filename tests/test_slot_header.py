"""The ordered slot sum of the parameter gradients is stated once (csrc/dq_slots.h): the reduce kernels call it, the
index-order sum has one launcher, and the kernels it replaced stay retired.  Reads the sources; no GPU, no build."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-deconvolution-dia-msms-data_amd", "csrc")


def _sources():
    return {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".cpp", ".h"))}


def _function_body(text, name):
    """the brace-balanced body of the function definition `name(...) {`"""
    m = re.search(r"\b" + name + r"\([^;{]*\)\s*\{", text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i]


def test_retired_reduce_kernels_are_gone():
    for name in ("k_wgrad_reduce_multi", "k_sum_b"):
        assert [n for n, text in _sources().items() if name in text] == [], name


def test_the_reduce_kernels_call_the_shared_slot_sum():
    texts = _sources()
    for n in ("k_la_reduce.hip", "k_conv.hip", "k_res_wg.hip"):
        assert "slot_sum<" in texts[n] and "slot_meet<" in texts[n] and '#include "dq_slots.h"' in texts[n], n
    # the two-accumulator loop itself lives in the header alone
    assert [n for n, text in texts.items() if re.search(r"s0 \+= \w+\[\(int64_t\)", text)] == ["dq_slots.h"]


def test_the_index_order_sum_has_one_launcher():
    texts = _sources()
    launch = r"hipLaunchKernelGGL\(\s*k_partial_reduce\b"
    assert [n for n, text in texts.items() if re.search(launch, text)] == ["k_tfm.hip"]
    assert len(re.findall(launch, texts["k_tfm.hip"])) == 1
    assert re.search(launch, _function_body(texts["k_tfm.hip"], "launch_ordered_sum"))
    assert "launch_ordered_sum(" in _function_body(texts["k_wide.hip"], "launch_sum_b")
