"""References for the evaluation of joint sampling: the numpy fp32 transcription of ``dq_mix_group_batch``'s rules,
which tests/test_group_batch.py holds the kernel to bit for bit, and a float64 statement of ``dq_group_metrics`` with the bound
tests/test_group_metrics.py asserts.  Built on the transcription of ``dq_mix_batch`` (tests/test_mix_host.py): the weights are the same
function, the products the same products."""
import numpy as np

from test_mix_host import mix_weights_ref

F32 = np.float32
GROUP_OUTS = ("ms2_target", "ms1_target", "ms2_cond", "ms2_rest", "weights_out")


def mix_group_batch_ref(ms2, ms1, idx, count, K, P, weights, E, seed, ids, draw, scale_target):
    """What dq_mix_group_batch writes: dict of ms2_target (P*G, RT, MZ), ms1_target (P*G, ...), ms2_cond (P*G, RT, MZ), ms2_rest (G, RT, MZ),
    weights_out (G, K), all float32, member-major (member p of group g is row p * G + g).  idx (K, G); count (G) or None; weights: K fixed
    floats or None (drawn under seed / ids (None: g) / draw).  A group with a count outside [P, K] or a used index outside the dataset is
    NaN in every output."""
    ms2, ms1 = np.asarray(ms2, dtype=F32), np.asarray(ms1, dtype=F32)
    n, G = len(ms2), idx.shape[1]
    counts = np.full(G, K) if count is None else np.asarray(count)
    if weights is None:
        w_all = mix_weights_ref(seed, range(G) if ids is None else ids, draw, np.clip(counts, 0, K), K, E)
    else:
        w_all = np.where(np.arange(K)[None, :] < counts[:, None], np.asarray(weights, dtype=F32)[None, :], F32(0)).astype(F32)
    out = {"ms2_target": np.empty((P * G,) + ms2.shape[1:], F32), "ms1_target": np.empty((P * G,) + ms1.shape[1:], F32),
           "ms2_cond": np.empty((P * G,) + ms2.shape[1:], F32), "ms2_rest": np.empty((G,) + ms2.shape[1:], F32), "weights_out": w_all.copy()}
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(G):
            c = int(counts[g])
            used = [int(idx[j, g]) for j in range(c)] if 0 <= c <= K else []  # rows j >= count are never read
            if not P <= c <= K or any(i < 0 or i >= n for i in used):
                for k in ("ms2_target", "ms1_target", "ms2_cond"):
                    out[k][g::G] = np.nan
                out["ms2_rest"][g] = np.nan
                out["weights_out"][g] = np.nan
                continue
            lo, hi = min(ms2[i].min() for i in used), max(ms2[i].max() for i in used)
            norm = [(ms2[i] - lo) / (hi - lo) for i in used]
            w = w_all[g]
            prod = [norm[j] * w[j] for j in range(c)]
            cond = prod[0]
            for j in range(1, c):
                cond = cond + prod[j]
            rest = np.zeros_like(cond)
            for j in range(P, c):
                rest = prod[j] if j == P else rest + prod[j]
            for p in range(P):
                lo1, hi1 = ms1[used[p]].min(), ms1[used[p]].max()
                out["ms2_target"][p * G + g] = prod[p] if scale_target else norm[p]
                out["ms1_target"][p * G + g] = (ms1[used[p]] - lo1) / (hi1 - lo1)
                out["ms2_cond"][p * G + g] = cond
            out["ms2_rest"][g] = rest
    assert all(v.dtype == F32 for v in out.values())
    return out


def group_metrics_ref(pred, target, mix, P):
    """float64: (cross (G, P, P), group (G, 3), bound_cross, bound_group) for pred / target (P*G, RT, MZ) and mix (G, RT, MZ).  The bounds
    are what tests/test_group_metrics.py allows the kernel's fp32 outputs around the float64 values: one fp32 rounding of the reference
    (2^-24 |ref|) plus n 2^-52 times the same ratio formed over absolute values -- the first-order error of an fp64 sum of n terms, each
    accumulated with at most n roundings, through a quotient."""
    pred, target, mix = (np.asarray(a, dtype=np.float64) for a in (pred, target, mix))
    G = mix.shape[0]
    n = mix[0].size
    pr, tg, mx = pred.reshape(P, G, n), target.reshape(P, G, n), mix.reshape(G, n)
    pp, tt = (pr * pr).sum(-1), (tg * tg).sum(-1)  # (P, G)
    cross, b_cross = np.zeros((G, P, P)), np.zeros((G, P, P))
    for g in range(G):
        for p in range(P):
            for q in range(P):
                if pp[p, g] > 0 and tt[q, g] > 0:
                    den = np.sqrt(pp[p, g] * tt[q, g])
                    cross[g, p, q] = (pr[p, g] * tg[q, g]).sum() / den
                    b_cross[g, p, q] = 2.0 ** -24 * abs(cross[g, p, q]) + n * 2.0 ** -52 * (np.abs(pr[p, g] * tg[q, g]).sum() / den)
    S, mp = np.maximum(pr, 0).sum(0), np.maximum(mx, 0)  # (G, n)
    tot = mp.sum(-1)
    group, b_group = np.zeros((G, 3)), np.zeros((G, 3))
    for g in range(G):
        group[g, 2] = tot[g]
        b_group[g, 2] = 2.0 ** -24 * tot[g] + n * 2.0 ** -52 * tot[g]
        if tot[g] > 0:
            group[g, 0] = np.maximum(S[g] - mp[g], 0).sum() / tot[g]
            group[g, 1] = np.maximum(mp[g] - S[g], 0).sum() / tot[g]
            # over absolute values: the terms |S - m+| are bounded by S + m+
            b_group[g, :2] = 2.0 ** -24 * group[g, :2] + n * 2.0 ** -52 * ((S[g] + mp[g]).sum() / tot[g])
    return cross, group, b_cross, b_group


def id_stats_ref(cross):
    """(id_acc, leak or None) of a (groups, P, P) cross matrix, written out member by member: a member is identified when the first
    maximum of its row sits on the diagonal; its leak is the largest off-diagonal entry of its row."""
    cross = np.asarray(cross, dtype=np.float64)
    n_groups, P, _ = cross.shape
    hits, leaks = [], []
    for g in range(n_groups):
        for p in range(P):
            row = cross[g, p]
            best = 0
            for q in range(1, P):
                if row[q] > row[best]:
                    best = q
            hits.append(best == p)
            if P > 1:
                leaks.append(max(row[q] for q in range(P) if q != p))
    return float(np.mean(hits)), (float(np.mean(leaks)) if P > 1 else None)
