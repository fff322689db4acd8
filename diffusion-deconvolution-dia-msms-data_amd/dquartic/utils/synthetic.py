"""Synthetic multiplexed-MS2 windows.  The reference ships no generator (its data come from
instrument files through an offline ETL); this one exists so that the hot path can be benchmarked and tested on data of
the right shape and statistics.

Window i (``rng = np.random.default_rng(1234 + i)``): K ~ U{3..12} co-eluting "peptides", each with an RT apex
~ U(0, RT), an elution width sigma ~ U(3, 15), F ~ U{4..12} fragment m/z bins ~ U{0..MZ-1} with LogNormal(0,1)
intensities; ``ms2[rt, mz] = sum_f I_f * exp(-(rt - apex)^2 / (2 sigma^2))`` and the MS1 chromatogram is the
precursor trace ``ms1[rt] = sum_k I_k * exp(...)``.  ``SyntheticDIAMSDataset`` then follows the reference dataset
contract (data_loader.py:60-90): ``__getitem__`` ignores its index, draws a random PAIR of windows, min-max
normalises the pair (MS2: min/max over both windows; MS1: min/max of window 1, applied to both) and returns
``(ms2_1, ms1_1, ms2_2, ms1_2)``; ``reset_epoch()`` exists because the harness calls it.

``ms1_channels=M1`` (optional) yields the MS1 slice the reference's data generator writes, ``(RT, M1)``: each peptide's precursor trace is
spread over ``M1`` isotope-like channels -- a first channel ~ U{0..M1-1} and up to four following ones with intensities falling by a
factor ~ U(0.3, 0.8) each.  These draws come from a generator of their own (seed ``987654 + i``), so the MS2 window and, without the
argument, the 1-D chromatogram are the same numbers as ever.
"""
import numpy as np
import torch
from torch.utils.data import Dataset


def make_window(i: int, RT: int = 400, MZ: int = 64, ms1_channels=None):
    rng = np.random.default_rng(1234 + i)
    rt = np.arange(RT, dtype=np.float32)[:, None]
    ms2 = np.zeros((RT, MZ), np.float32)
    M1 = None if ms1_channels is None else int(ms1_channels)
    if M1 is not None and M1 < 1:
        raise ValueError("ms1_channels must be >= 1")
    ms1 = np.zeros((RT,) if M1 is None else (RT, M1), np.float32)
    rng1 = None if M1 is None else np.random.default_rng(987654 + i)  # (its own stream: the draws above and below stay what they were)
    for _ in range(int(rng.integers(3, 13))):
        apex = rng.uniform(0, RT)
        sigma = rng.uniform(3, 15)
        prof = np.exp(-((rt - apex) ** 2) / (2 * sigma * sigma)).astype(np.float32)  # (RT, 1)
        nfrag = int(rng.integers(4, 13))
        bins = rng.integers(0, MZ, size=nfrag)
        inten = rng.lognormal(0.0, 1.0, size=nfrag).astype(np.float32)
        np.add.at(ms2, (slice(None), bins), prof * inten[None, :])
        inten1 = float(rng.lognormal(0.0, 1.0))
        if M1 is None:
            ms1 += inten1 * prof[:, 0]
        else:  # the precursor's isotope envelope: consecutive channels, falling intensities
            first = int(rng1.integers(0, M1))
            for k in range(min(5, M1 - first)):
                ms1[:, first + k] += np.float32(inten1) * prof[:, 0]
                inten1 *= float(rng1.uniform(0.3, 0.8))
    return ms2, ms1


def make_pool(n: int, RT: int = 400, MZ: int = 64, start: int = 0, ms1_channels=None):
    ms2 = np.empty((n, RT, MZ), np.float32)
    ms1 = np.empty((n, RT) if ms1_channels is None else (n, RT, int(ms1_channels)), np.float32)
    for i in range(n):
        ms2[i], ms1[i] = make_window(start + i, RT, MZ, ms1_channels)
    return ms2, ms1


def normalize_pair(ms2_1, ms1_1, ms2_2, ms1_2):
    """Per-pair min-max exactly as data_loader.py:70-79 (MS1 statistics come from window 1 only)."""
    lo, hi = min(ms2_1.min(), ms2_2.min()), max(ms2_1.max(), ms2_2.max())
    ms2_1, ms2_2 = (ms2_1 - lo) / (hi - lo), (ms2_2 - lo) / (hi - lo)
    lo1, hi1 = ms1_1.min(), ms1_1.max()
    ms1_1, ms1_2 = (ms1_1 - lo1) / (hi1 - lo1), (ms1_2 - lo1) / (hi1 - lo1)
    return ms2_1, ms1_1, ms2_2, ms1_2


class SyntheticDIAMSDataset(Dataset):
    def __init__(self, n_windows: int = 32, RT: int = 400, MZ: int = 64, normalize="minmax", seed: int = 0, rank: int = 0, world: int = 1,
                 ms1_channels=None, start: int = 0):
        if normalize is None:
            raise ValueError("normalize must be 'minmax' (the reference raises on None, data_loader.py:80-81)")
        # rank r of `world` owns windows i with i % world == r; `start` shifts the pool (a held-out set: windows the
        # training pool 0 .. n_windows-1 does not contain)
        ids = [int(start) + i for i in range(n_windows) if i % world == rank]
        self.ms2 = np.stack([make_window(i, RT, MZ)[0] for i in ids])
        self.ms1 = np.stack([make_window(i, RT, MZ, ms1_channels)[1] for i in ids])
        self.normalize = normalize
        self._rng = np.random.default_rng(seed + 7919 * rank)

    def __len__(self):
        return len(self.ms2)

    def reset_epoch(self):
        pass

    def __getitem__(self, idx):
        a, b = self._rng.choice(len(self.ms2), size=2, replace=len(self.ms2) < 2)
        return self.pair(a, b)

    def valid_pair(self, a, b) -> bool:
        return a != b or len(self.ms2) < 2

    def pair(self, a, b):
        """The normalised item of the windows (a, b) of the pool."""
        out = normalize_pair(self.ms2[a], self.ms1[a], self.ms2[b], self.ms1[b])
        return tuple(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for v in out)


class FrozenPairDataset(Dataset):
    """A held-out set: ``n_pairs`` named pairs of ``dataset``'s windows.  The reference's dataset contract ignores the index and returns a
    fresh random pair on every access, drawn from a process-wide generator (data_loader.py:60-69) -- what training wants and what a
    held-out set must not do.  Here the index pairs ``(i, j)`` are drawn once from a generator of their own,
    ``numpy.random.default_rng(seed)``, so they depend on ``(len(dataset), n_pairs, seed)`` and on nothing else: the same pairs in the
    same order in every process, every run and every restart, which is what makes two ``evaluate`` runs comparable.  Item k is
    ``dataset.pair(*index_pairs[k])``, formed on access: nothing is kept in host memory but the indices.  ``dataset`` needs ``pair(i,
    j)`` and ``valid_pair(i, j)`` (``DIAMSDataset``, ``SyntheticDIAMSDataset``).  ``n_pairs`` None: one pair per window of the dataset."""

    def __init__(self, dataset, n_pairs=None, seed: int = 0):
        n_windows = len(dataset)
        n = n_windows if n_pairs is None else int(n_pairs)
        if n < 1 or n_windows < 1:
            raise ValueError(f"FrozenPairDataset: need at least one pair and one window, got {n} pairs of {n_windows} windows")
        rng = np.random.default_rng(int(seed))
        self.dataset, self.seed, self.index_pairs = dataset, int(seed), []
        tries = 0
        while len(self.index_pairs) < n:
            i, j = (int(v) for v in rng.integers(0, n_windows, size=2))
            tries += 1
            if dataset.valid_pair(i, j):
                self.index_pairs.append((i, j))
            elif tries > 1000 * n + 1000:
                raise ValueError("FrozenPairDataset: the dataset has no two windows that may form a pair")

    def __len__(self):
        return len(self.index_pairs)

    def __getitem__(self, idx):
        return self.dataset.pair(*self.index_pairs[idx])
