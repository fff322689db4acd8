#!/usr/bin/env python3
"""Which kernel form every shape takes, as the library's device-free query entries answer it, written to one JSON file of integer arrays,
and the entry-for-entry comparison of such a file with what the loaded library answers now (the instantiation tables
of csrc/k_*.hip decide these answers; tests/golden/launch_forms.json pins them).

    DQ_HIP_LIB=<library> python tools/launch_forms.py dump out.json
    DQ_HIP_LIB=<library> python tools/launch_forms.py compare tests/golden/launch_forms.json      (exit status 1 on a difference)

Swept: dq_resblock_forms, dq_linattn_forms and dq_conv_bwd_forms over C in {4, 8, 12, 16}, skip / stage widths C - 8 .. C + 8 (steps of 4,
clipped to 0 .. 16: pairs that are not built are pinned too), n in {1, 2, 4, .., 1024} and rows_per_sample in {1, 3, 400} at 2 and at 64
samples; dq_debug_level_plan and dq_debug_mid_forms over the networks of tests/test_level_plan.py at B in {1, 32}.  The three row-count
options are set to 0 and to 2^30 around the sweeps they can touch, so that no answer depends on a compute-unit count.  An entry that the
library refuses is recorded as -1.  Values are form indices (include/dq_hip.h), two forms packed as 16 * first + second."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CS = (4, 8, 12, 16)
NS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
ROWS = [(rps, rps * b) for b in (2, 64) for rps in (1, 3, 400)]  # (rows_per_sample, rows)
OPTIONS = ("res_rows_bwd_min_rows", "la_small_min_rows", "la_rows_bwd_min_rows")
CONVS = ((1, 0), (3, 0), (7, 0), (4, 1), (3, 2))  # (K, mode): CONV_S1 = 0 | CONV_DOWN = 1 | CONV_UP = 2 (csrc/dq_kernels.h)


def widths(C, lo=0):
    return [w for w in range(C - 8, C + 9, 4) if lo <= w <= 16]


def sweep():
    import test_level_plan as TP
    from dquartic import _native as N

    L = N.lib()
    f, g = ctypes.c_int(), ctypes.c_int()

    def pair(rc):
        return 16 * f.value + g.value if rc == 0 else -1

    out = {}
    saved = {k: N.get_option(k) for k in OPTIONS}
    try:
        for thr in (0, 1 << 30):
            for k in OPTIONS:
                N.set_option(k, thr)
            # a block of C channels behind cat(x, skip), and a block from another width without a skip
            out[f"resblock/min_rows={thr}"] = [
                pair(L.dq_resblock_forms(cinA, cinB, C, rows, n, rps, ctypes.byref(f), ctypes.byref(g)))
                for C in CS for cinA, cinB in [(C, w) for w in widths(C)] + [(w, 0) for w in widths(C, 4) if w != C]
                for n in NS for rps, rows in ROWS]
            out[f"linattn/min_rows={thr}"] = [
                pair(L.dq_linattn_forms(C, rows, n, prepared, ctypes.byref(f), ctypes.byref(g)))
                for C in CS for n in NS for _, rows in ROWS for prepared in (0, 1)]
    finally:
        for k, v in saved.items():
            N.set_option(k, v)
    # (n = the output's row length; the input's follows from the mode)
    out["conv_bwd"] = [
        pair(L.dq_conv_bwd_forms(C, cp, 0, K, mode, rows, (n, 2 * n, n // 2)[mode], n, rps, bias, aligned, ctypes.byref(f), ctypes.byref(g)))
        for C in CS for cp in widths(C, 4) for K, mode in CONVS for n in NS if not (mode == 2 and n < 2)
        for rps, rows in ROWS for bias in (0, 1) for aligned in (0, 1)]
    for cfg in sorted(TP.CONFIGS):
        plan = TP._make_plan(cfg)
        try:
            for B in (1, 32):
                cap = 1 + len(N.LEVEL_FORM_FIELDS) * 21 + len(N.LEVEL_PLAN_FLAGS)
                buf = (ctypes.c_int32 * cap)()
                for save in (0, 1):
                    for twin in (0, 1):
                        n = L.dq_debug_level_plan(plan, B, 37, save, twin, buf, cap)
                        out[f"level_plan/{cfg}/B={B}/save={save}/twin={twin}"] = [int(v) for v in buf[:n]] if n > 0 else [-1]
                mbuf = (ctypes.c_int32 * len(N.MID_FORMS_FIELDS))()
                n = L.dq_debug_mid_forms(plan, B, 37, mbuf, len(N.MID_FORMS_FIELDS))
                out[f"mid_forms/{cfg}/B={B}"] = [int(v) for v in mbuf[:n]] if n > 0 else [-1]
        finally:
            L.dq_plan_destroy(plan)
    return out


def differences(golden, now):
    diffs = [f"{k}: only in one of the two" for k in sorted(set(golden) ^ set(now))]
    for k in sorted(set(golden) & set(now)):
        a, b = golden[k], now[k]
        if len(a) != len(b):
            diffs.append(f"{k}: {len(a)} entries against {len(b)}")
        diffs += [f"{k}[{i}]: {x} against {y}" for i, (x, y) in enumerate(zip(a, b)) if x != y]
    return diffs


def main(argv):
    if len(argv) != 3 or argv[1] not in ("dump", "compare"):
        print(__doc__)
        return 2
    now = sweep()
    if argv[1] == "dump":
        with open(argv[2], "w") as fh:
            json.dump(now, fh, separators=(",", ":"), sort_keys=True)
            fh.write("\n")
        print(f"{argv[2]}: {sum(len(v) for v in now.values())} entries in {len(now)} arrays")
        return 0
    with open(argv[2]) as fh:
        diffs = differences(json.load(fh), now)
    for d in diffs:
        print(d)
    print(f"{len(diffs)} differences")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
