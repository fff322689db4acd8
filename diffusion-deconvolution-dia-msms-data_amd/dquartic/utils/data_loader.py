"""``DIAMSDataset`` -- same contract as the reference's ``dquartic/utils/data_loader.py`` (:10-185): ``__getitem__`` ignores
its index, draws a random PAIR of distinct windows not yet used this epoch, min-max normalises the pair (MS2 over both
windows, MS1 from window 1 only; :70-79) and returns ``(ms2_1, ms1_1, ms2_2, ms1_2)`` as float32 tensors;
``reset_epoch()`` clears the used-pair set.  Backends: two ``.npy`` files (mmap) or a directory of parquet slices with the
schema the reference's ETL writes (data_generation.py:206-223).  The parquet backend uses pyarrow (duckdb is not a
dependency here); slices are addressed by (file, row) instead of a six-column SQL filter, same result."""
import glob
import os
import random
from typing import Literal

import numpy as np
import torch
from torch.utils.data import Dataset


class DIAMSDataset(Dataset):
    def __init__(self, parquet_directory=None, ms2_file=None, ms1_file=None, normalize: Literal[None, "minmax"] = None):
        if parquet_directory is None and ms1_file is not None and ms2_file is not None:
            self.ms2_data = np.load(ms2_file, mmap_mode="r")
            self.ms1_data = np.load(ms1_file, mmap_mode="r")
            self.data_type = "npy"
            print(f"Info: Loaded  {len(self.ms2_data)} MS2 slice samples and {len(self.ms1_data)} MS1 slice samples from NPY files.")
        elif parquet_directory is not None and ms1_file is None and ms2_file is None:
            self.parquet_directory = parquet_directory
            self.meta = self.read_parquet_meta(parquet_directory)
            self.data_type = "parquet"
            print(f"Info: Loaded {len(self.meta)} MS2 slice samples and MS1 slice samples from Parquet files.")
        else:
            raise ValueError("Invalid input data arguments. Please provide either a `parquet_directory` or `ms2_file` and `ms1_file`. "
                             f"Got parquet_directory={parquet_directory}, ms2_file={ms2_file}, ms1_file={ms1_file}.")
        self.normalize = normalize
        self.used_pairs = set()
        self.epoch_reset = False

    def __len__(self):
        return len(self.meta) if self.data_type == "parquet" else len(self.ms2_data)

    def reset_epoch(self):
        self.used_pairs.clear()
        self.epoch_reset = True

    # ---- parquet backend
    def read_parquet_meta(self, parquet_directory):
        import pyarrow.parquet as pq

        meta = []
        for path in sorted(glob.glob(os.path.join(parquet_directory, "*.parquet"))):
            t = pq.read_table(path, columns=["slice_index", "mz_isolation_target"])
            si, mt = t.column("slice_index").to_pylist(), t.column("mz_isolation_target").to_pylist()
            meta.extend((path, i, si[i], mt[i]) for i in range(len(si)))
        return meta

    def _get_parquet_data(self, entry):
        import pyarrow.parquet as pq

        path, row, _, _ = entry
        t = pq.read_table(path, columns=["ms2_data", "ms1_data", "ms2_shape", "ms1_shape"]).slice(row, 1).to_pylist()[0]
        ms2 = np.asarray(t["ms2_data"], dtype=np.float32).reshape(t["ms2_shape"])
        ms1 = np.asarray(t["ms1_data"], dtype=np.float32).reshape(t["ms1_shape"])
        return ms1, ms2

    # ---- pair sampling
    def _draw_pair(self, n, same=None):
        if n < 2:
            raise ValueError("DIAMSDataset needs at least two windows to form a pair")
        if len(self.used_pairs) >= n * (n - 1) // 2:
            self.used_pairs.clear()  # every pair used: start over instead of spinning forever
        while True:
            i, j = random.randint(0, n - 1), random.randint(0, n - 1)
            if i == j or (same is not None and same(i, j)):
                continue
            pair = (min(i, j), max(i, j))
            if pair in self.used_pairs:
                continue
            self.used_pairs.add(pair)
            return i, j

    def valid_pair(self, i, j) -> bool:
        """May windows i and j form a pair?  Distinct, and (parquet) not the same slice of the same isolation target."""
        if i == j:
            return False
        return self.data_type == "npy" or not (self.meta[i][2] == self.meta[j][2] and self.meta[i][3] == self.meta[j][3])

    def __getitem__(self, idx):
        if self.data_type == "npy":
            i, j = self._draw_pair(len(self.ms2_data))
        else:
            same = lambda a, b: self.meta[a][2] == self.meta[b][2] and self.meta[a][3] == self.meta[b][3]
            i, j = self._draw_pair(len(self.meta), same)
        return self.pair(i, j)

    def pair(self, i, j):
        """The normalised item of the windows (i, j): what ``__getitem__`` returns for the pair it drew (a held-out set names its pairs)."""
        if self.data_type == "npy":
            ms2_1, ms1_1, ms2_2, ms1_2 = self.ms2_data[i], self.ms1_data[i], self.ms2_data[j], self.ms1_data[j]
        else:
            ms1_1, ms2_1 = self._get_parquet_data(self.meta[i])
            ms1_2, ms2_2 = self._get_parquet_data(self.meta[j])
        if self.normalize == "minmax":
            lo, hi = min(ms2_1.min(), ms2_2.min()), max(ms2_1.max(), ms2_2.max())
            lo1, hi1 = ms1_1.min(), ms1_1.max()
            ms2_1, ms2_2 = (ms2_1 - lo) / (hi - lo), (ms2_2 - lo) / (hi - lo)
            ms1_1, ms1_2 = (ms1_1 - lo1) / (hi1 - lo1), (ms1_2 - lo1) / (hi1 - lo1)
        else:
            raise ValueError("Invalid normalization method. Valid options are: None, 'minmax'.")
        return tuple(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for v in (ms2_1, ms1_1, ms2_2, ms1_2))


# ----------------------------------------------------------------------------------------------------------------------
# HBM-resident batch formation: not in the reference -- at ~2,500 windows/s per GPU the per-item numpy
# min-max + collate + H2D copy of a DataLoader becomes the bottleneck, so the whole dataset lives in HBM (288 GB hold
# ~2.8 M windows of 400 x 64) and a batch is formed by one native call (csrc/k_pairs.hip: dq_pair_batch).
# ----------------------------------------------------------------------------------------------------------------------
def _resident_tensors(dataset_or_arrays, device):
    """The windows a resident loader keeps in HBM: ``(ms2 (N, RT, MZ), ms1 (N, ...))`` as float32 device tensors, from a ``DIAMSDataset``
    (npy: its arrays; parquet: every slice materialised once), a dataset that holds ``ms2`` / ``ms1`` arrays (``SyntheticDIAMSDataset``)
    or an ``(ms2, ms1)`` pair of arrays.  A dataset must normalise by "minmax", the one rule the kernels implement."""
    import warnings

    ds = dataset_or_arrays
    if isinstance(ds, (tuple, list)):
        ms2, ms1 = (np.asarray(a) for a in ds)
    else:
        if getattr(ds, "normalize", None) != "minmax":
            raise ValueError("Invalid normalization method. Valid options are: None, 'minmax'.")  # data_loader.py:81
        if getattr(ds, "data_type", None) == "parquet":
            rows = [ds._get_parquet_data(e) for e in ds.meta]
            ms1, ms2 = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        elif hasattr(ds, "ms2_data"):
            ms2, ms1 = np.asarray(ds.ms2_data), np.asarray(ds.ms1_data)
        else:
            ms2, ms1 = np.asarray(ds.ms2), np.asarray(ds.ms1)
    if ms2.ndim != 3 or len(ms1) != len(ms2):
        raise ValueError(f"expected ms2 (N, RT, MZ) and ms1 (N, ...), got {ms2.shape} and {ms1.shape}")
    with warnings.catch_warnings():  # read-only mmap views are only read (uploaded) here
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        return (torch.from_numpy(np.ascontiguousarray(ms2, dtype=np.float32)).to(device),
                torch.from_numpy(np.ascontiguousarray(ms1, dtype=np.float32)).to(device))


class PairBatch(tuple):
    """``(ms2_1, ms1_1, ms2_2, ms1_2)`` -- what a ``DataLoader(DIAMSDataset)`` batch unpacks to -- already on the device,
    plus ``ms2_cond`` = the mixture for ``mixture_weights`` (formed in the same kernel)."""

    def __new__(cls, items, ms2_cond, mixture_weights):
        self = super().__new__(cls, items)
        self.ms2_cond = ms2_cond
        self.mixture_weights = tuple(float(w) for w in mixture_weights)
        return self


class ResidentPairLoader:
    """Drop-in for ``DataLoader(DIAMSDataset(...), batch_size=B)`` that keeps the windows in HBM.

    Pairs are drawn on the host by ``dataset._draw_pair`` -- the reference's rule (data_loader.py:118-131: two
    ``random.randint`` per attempt, distinct windows, unused this epoch) consuming the same ``random`` stream as iterating
    the reference dataset in one process; the gather, the per-pair min-max (:70-79) and the mixture
    (model_interface.py:1073-1075) run in ``dq_pair_batch``.  One epoch = ``len(dataset) // world_size`` pairs, like a
    (distributed) sampler over a dataset whose ``__getitem__`` ignores its index.  Arithmetic is fp32: float64 source
    arrays are converted once at upload (the reference normalises in the source dtype and casts afterwards)."""

    def __init__(self, dataset, batch_size, device="cuda", mixture_weights=(0.5, 0.5), drop_last=False, rank=0, world_size=1):
        from .. import _native as N

        self._N = N
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        self.mixture_weights = tuple(float(w) for w in mixture_weights)
        self.drop_last, self.rank, self.world_size = bool(drop_last), int(rank), int(world_size)
        self._same = None
        if getattr(dataset, "data_type", "npy") != "npy":  # parquet backend: never the same slice of the same isolation target
            meta = dataset.meta
            self._same = lambda a, b: meta[a][2] == meta[b][2] and meta[a][3] == meta[b][3]
        N.lib()  # fail loudly now if the native library is missing
        self.ms2, self.ms1 = _resident_tensors(dataset, self.device)
        self.n, self.RT, self.MZ = self.ms2.shape
        self.ms1_shape = tuple(self.ms1.shape[1:])
        self.ms1_per = int(np.prod(self.ms1_shape)) if self.ms1_shape else 1
        self._scratch = torch.empty(max(1, N.lib().dq_pair_batch_scratch_bytes(self.batch_size) // 4), dtype=torch.float32, device=self.device)

    def _items(self):
        return max(1, len(self.dataset) // self.world_size)

    def __len__(self):
        n = self._items()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def form(self, idx1, idx2):
        """One native call for explicit index lists -> PairBatch (also the parity-test entry)."""
        N = self._N
        B = len(idx1)
        if B != len(idx2) or B == 0 or B > self.batch_size:
            raise ValueError(f"need 1..{self.batch_size} index pairs, got {len(idx1)} and {len(idx2)}")
        idx = torch.tensor(list(idx1) + list(idx2), dtype=torch.int64).to(self.device, non_blocking=True)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        a, b, c = new(B, self.RT, self.MZ), new(B, self.RT, self.MZ), new(B, self.RT, self.MZ)
        m1, m2 = new(B, *self.ms1_shape), new(B, *self.ms1_shape)
        N.check(N.lib().dq_pair_batch(N.ptr(self.ms2), N.ptr(self.ms1), self.n, N.ptr(idx), B, self.RT, self.MZ, self.ms1_per,
                                      self.mixture_weights[0], self.mixture_weights[1], N.ptr(a), N.ptr(m1), N.ptr(b), N.ptr(m2), N.ptr(c),
                                      N.ptr(self._scratch), self._scratch.numel() * 4, N.stream_ptr()), "dq_pair_batch")
        return PairBatch((a, m1, b, m2), c, self.mixture_weights)

    def __iter__(self):
        left = self._items()
        while left > 0:
            B = min(self.batch_size, left)
            if B < self.batch_size and self.drop_last:
                return
            pairs = [self.dataset._draw_pair(self.n, self._same) for _ in range(B)]
            left -= B
            yield self.form([p[0] for p in pairs], [p[1] for p in pairs])


# ----------------------------------------------------------------------------------------------------------------------
# K-component mixtures with per-window weights (csrc/k_mix.hip: dq_mix_batch).  Not in the reference, whose
# mixture is one pair at (0.5, 0.5): a window here mixes 1..K distinct windows of the resident dataset at abundances drawn on
# the device, and the target is the first component's CONTRIBUTION to the mixture.
# ----------------------------------------------------------------------------------------------------------------------
MIX_MAX_COMPONENTS = 8  # dq_mix_batch: K in 2..8


def _mix_components(n_components, n_windows=None):
    """``(kmin, kmax)`` of an ``n_components`` argument, checked: 1 <= kmin <= kmax, 2 <= kmax <= 8 (the rule of the ``data.mixture``
    config block: K = kmax is the kernel's K), and, given ``n_windows``, enough windows for kmax distinct ones."""
    kmin, kmax = (int(v) for v in n_components)
    if not (1 <= kmin <= kmax and 2 <= kmax <= MIX_MAX_COMPONENTS):
        raise ValueError(f"n_components must satisfy 1 <= kmin <= kmax and 2 <= kmax <= {MIX_MAX_COMPONENTS}, got {(kmin, kmax)}")
    if n_windows is not None and n_windows < kmax:
        raise ValueError(f"a mixture of {kmax} distinct windows needs at least {kmax} windows, got {n_windows}")
    return kmin, kmax


def draw_mix_indices(n_windows, n_items, n_components, rng, valid_pair=None):
    """Which windows form each of ``n_items`` mixtures: ``(idx, count)`` with ``idx`` int64 ``(K, n_items)`` (row j = component j, row 0
    the target) and ``count`` int32 ``(n_items,)``.  ``n_components = (kmin, kmax)``, K = kmax.  Per item, from ``rng`` (a
    ``numpy.random.Generator``) in this order: the count, uniform in [kmin, kmax]; the target, uniform over the windows; then component
    after component, redrawn until it differs from every earlier one of the item and ``valid_pair(target, j)`` holds (None: any distinct
    window).  Rows ``j >= count`` hold -1: the kernel never reads them, and whatever would is refused by its bounds check.  A pure host
    function of its arguments."""
    n_windows, n_items = int(n_windows), int(n_items)
    kmin, kmax = _mix_components(n_components, n_windows)
    if n_items < 1:
        raise ValueError(f"need at least one item, got {n_items}")
    idx = np.full((kmax, n_items), -1, dtype=np.int64)
    count = np.empty(n_items, dtype=np.int32)
    for b in range(n_items):
        count[b] = int(rng.integers(kmin, kmax + 1))
        for _ in range(100):  # a target that finds its partners within 100 tries each, another target otherwise
            comp = [int(rng.integers(0, n_windows))]
            tries = 0
            while len(comp) < count[b] and tries < 100 * kmax:
                j = int(rng.integers(0, n_windows))
                tries += 1
                if j not in comp and (valid_pair is None or valid_pair(comp[0], j)):
                    comp.append(j)
            if len(comp) == count[b]:
                break
        else:
            raise ValueError(f"draw_mix_indices: found no window with {int(count[b]) - 1} windows it may be mixed with")
        idx[:count[b], b] = comp
    return idx, count


class MixBatch(PairBatch):
    """``(ms2_target, ms1_target, ms2_rest, None)`` on the device: where a pair batch has the target window, its MS1, the other window
    and that one's MS1, this has the target (scaled by its weight under ``scale_target``), its MS1, the weighted sum of everything else,
    and nothing.  ``ms2_cond`` is the mixture, ``weights`` the ``(B, K)`` tensor of every window's w_j (0 for absent components), and
    ``mixture_final`` says that the mixture is not to be formed again from the items (``ModelInterface._batch_inputs``)."""

    mixture_final = True

    def __new__(cls, items, ms2_cond, weights):
        self = super().__new__(cls, items, ms2_cond, ())
        self.weights = weights
        return self


class ResidentMixLoader:
    """Batches of K-component mixtures from a dataset held in HBM, one ``dq_mix_batch`` call each.

    ``dataset_or_arrays``: a ``DIAMSDataset`` (npy or parquet), a ``SyntheticDIAMSDataset``, or an ``(ms2, ms1)`` pair of arrays
    ``(N, RT, MZ)`` / ``(N, ...)``.  ``n_components = (kmin, kmax)``: every window mixes a count of distinct windows uniform in that range
    (``draw_mix_indices``; pairs obey the dataset's ``valid_pair``).  ``weights`` None: the kernel draws them, uniformly within an octave
    and over ``max_ratio_log2`` octaves, normalised to sum 1 (so max w / min w < 2 ** max_ratio_log2); otherwise kmax fixed
    weights, used as they are.  ``scale_target``: the target is ``n_0 * w_0``, the first component's contribution to the mixture, rather
    than ``n_0``.

    Training form (``frozen_items`` None): one epoch = ``len(dataset) // world_size`` windows; the indices come from a host generator of
    ``(seed, rank)`` that runs on from epoch to epoch, the weights from ``seed + rank`` with the running batch number as the draw index
    and the batch positions as ids.  A loader built again with the same arguments yields the same batches.
    Held-out form (``frozen_items = n``): the indices of n items are drawn once from ``numpy.random.default_rng(seed)``; item k draws its
    weights under id k at draw 0 -- the same set in every run, every process and at every batch size."""

    def __init__(self, dataset_or_arrays, batch_size, n_components=(2, 4), max_ratio_log2=3, seed=0, scale_target=True, weights=None,
                 frozen_items=None, device="cuda", drop_last=False, rank=0, world_size=1):
        from .. import _native as N

        ds = dataset_or_arrays
        self._valid = None if isinstance(ds, (tuple, list)) else ds.valid_pair
        kmin, kmax = _mix_components(n_components)
        self.n_components, self.K = (kmin, kmax), kmax
        self.max_ratio_log2 = int(max_ratio_log2)
        if not 0 <= self.max_ratio_log2 <= 16:
            raise ValueError(f"max_ratio_log2 must be 0..16, got {max_ratio_log2}")
        if weights is not None and len(weights) != self.K:
            raise ValueError(f"weights: need {self.K} fixed weights, got {len(weights)}")
        self.weights = None if weights is None else tuple(float(w) for w in weights)
        self._N = N
        self.dataset, self.batch_size, self.device = ds, int(batch_size), torch.device(device)
        if not 1 <= self.batch_size <= 65535:
            raise ValueError(f"batch_size must be 1..65535, got {batch_size}")
        self.seed, self.scale_target = int(seed), bool(scale_target)
        self.drop_last, self.rank, self.world_size = bool(drop_last), int(rank), int(world_size)
        N.lib()  # fail loudly now if the native library is missing
        self.ms2, self.ms1 = _resident_tensors(ds, self.device)
        _mix_components(n_components, len(self.ms2))
        self.n, self.RT, self.MZ = self.ms2.shape
        self.ms1_shape = tuple(self.ms1.shape[1:])
        self.ms1_per = int(np.prod(self.ms1_shape)) if self.ms1_shape else 1
        self._scratch = torch.empty(max(1, N.lib().dq_mix_batch_scratch_bytes(self.batch_size, self.K) // 4), dtype=torch.float32,
                                    device=self.device)
        self.frozen = None
        if frozen_items is not None:
            self.frozen = draw_mix_indices(self.n, int(frozen_items), self.n_components, np.random.default_rng(self.seed), self._valid)
            weight_seed = self.seed
        else:
            self._rng = np.random.default_rng((self.seed, self.rank))
            weight_seed = self.seed + self.rank
        weight_seed &= 2 ** 64 - 1
        self._seed_dev = torch.tensor([weight_seed - 2 ** 64 if weight_seed >= 2 ** 63 else weight_seed], dtype=torch.int64, device=self.device)
        self._draw = 0  # the running batch number of the training form

    def _items(self):
        return self.frozen[0].shape[1] if self.frozen is not None else max(1, len(self.ms2) // self.world_size)

    def __len__(self):
        n = self._items()
        return n // self.batch_size if self.drop_last and self.frozen is None else (n + self.batch_size - 1) // self.batch_size

    def form(self, idx, count=None, draw=0, window_ids=None):
        """One native call for explicit indices ``(K, B)`` and counts ``(B,)`` (None: K everywhere) -> ``MixBatch``."""
        N = self._N
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.ndim != 2 or idx.shape[0] != self.K or not 1 <= idx.shape[1] <= self.batch_size:
            raise ValueError(f"need a ({self.K}, 1..{self.batch_size}) index array, got shape {idx.shape}")
        B = idx.shape[1]
        idx_dev = torch.from_numpy(idx).to(self.device, non_blocking=True)
        count_dev = None if count is None else torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(self.device, non_blocking=True)
        if count_dev is not None and count_dev.shape != (B,):
            raise ValueError(f"need {B} counts, got shape {tuple(count_dev.shape)}")
        ids_dev = None if window_ids is None else torch.as_tensor(np.ascontiguousarray(window_ids, dtype=np.int64)).to(self.device, non_blocking=True)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        tgt, cond, rest = new(B, self.RT, self.MZ), new(B, self.RT, self.MZ), new(B, self.RT, self.MZ)
        m1, w = new(B, *self.ms1_shape), new(B, self.K)
        import ctypes

        fixed = None if self.weights is None else (ctypes.c_float * self.K)(*self.weights)
        N.check(N.lib().dq_mix_batch(N.ptr(self.ms2), N.ptr(self.ms1), self.n, N.ptr(idx_dev), N.ptr(count_dev), B, self.K, self.RT, self.MZ,
                                     self.ms1_per, fixed, self.max_ratio_log2, N.ptr(self._seed_dev), N.ptr(ids_dev), int(draw),
                                     int(self.scale_target), N.ptr(tgt), N.ptr(m1), N.ptr(cond), N.ptr(rest), N.ptr(w),
                                     N.ptr(self._scratch), self._scratch.numel() * 4, N.stream_ptr()), "dq_mix_batch")
        return MixBatch((tgt, m1, rest, None), cond, w)

    def __iter__(self):
        if self.frozen is not None:
            idx, count = self.frozen
            for first in range(0, idx.shape[1], self.batch_size):
                last = min(first + self.batch_size, idx.shape[1])
                yield self.form(idx[:, first:last], count[first:last], draw=0, window_ids=np.arange(first, last, dtype=np.int64))
            return
        left = self._items()
        while left > 0:
            B = min(self.batch_size, left)
            if B < self.batch_size and self.drop_last:
                return
            idx, count = draw_mix_indices(self.n, B, self.n_components, self._rng, self._valid)
            left -= B
            batch = self.form(idx, count, draw=self._draw)
            self._draw += 1
            yield batch


# ----------------------------------------------------------------------------------------------------------------------
# Groups: one mixture, P targets (csrc/k_mix.hip: dq_mix_group_batch).  What joint sampling (section 40) is scored
# on: the first P components of a mixture are the members that ``sample(group_size=P)`` is asked for, each with its own target and MS1.
# ----------------------------------------------------------------------------------------------------------------------
class GroupBatch(MixBatch):
    """A ``MixBatch`` whose items are member-major: ``(ms2_target (P*G, RT, MZ), ms1_target (P*G, ...), ms2_rest (G, RT, MZ), None)`` with
    member p of group g in row ``p * G + g`` -- the layout ``sample(group_size=P)`` takes.  ``ms2_cond`` ``(P*G, RT, MZ)`` repeats the
    group's mixture in every member's slice, ``weights`` is ``(G, K)`` (one mixture per group), ``rest`` the part of the mixture that no
    member explains (0 where the group has exactly P components) and ``group_size`` P."""

    def __new__(cls, items, ms2_cond, weights, group_size):
        self = super().__new__(cls, items, ms2_cond, weights)
        self.group_size = int(group_size)
        self.rest = items[2]
        return self

    @property
    def n_groups(self):
        return self[0].shape[0] // self.group_size

    def member_weights(self):
        """``(P*G,)``: every member's own share w_p of its group's mixture, member-major"""
        return self.weights[:, :self.group_size].t().reshape(-1)


class ResidentGroupLoader(ResidentMixLoader):
    """``ResidentMixLoader`` for groups: batches of ``groups_per_batch`` mixtures whose first ``group_size`` components are the members,
    one ``dq_mix_group_batch`` call each.  The arguments and their rules are ``ResidentMixLoader``'s, with
    ``group_size <= kmin`` on top (every mixture must hold its members).  The indices and the weights are drawn exactly as that loader draws
    them, so with ``frozen_items`` group k IS item k of a ``ResidentMixLoader`` built with the same arguments: the same mixture, the same
    weights, and member 0 is that loader's window bit for bit; members 1 .. P-1 are the next components of the same mixture, each with the
    target and the MS1 it would have as the target of its own window."""

    def __init__(self, dataset_or_arrays, groups_per_batch, group_size, n_components=(2, 4), max_ratio_log2=3, seed=0, scale_target=True,
                 weights=None, frozen_items=None, device="cuda", drop_last=False, rank=0, world_size=1):
        kmin, _ = _mix_components(n_components)
        if isinstance(group_size, bool) or not isinstance(group_size, (int, np.integer)) or not 1 <= int(group_size) <= kmin:
            raise ValueError(f"group_size must be an integer in [1, kmin = {kmin}] (every mixture holds its members), got {group_size!r}")
        super().__init__(dataset_or_arrays, groups_per_batch, n_components=n_components, max_ratio_log2=max_ratio_log2, seed=seed,
                         scale_target=scale_target, weights=weights, frozen_items=frozen_items, device=device, drop_last=drop_last, rank=rank,
                         world_size=world_size)
        self.group_size = int(group_size)
        self._group_scratch = torch.empty(max(1, self._N.lib().dq_mix_group_batch_scratch_bytes(self.batch_size, self.K, self.group_size) // 4),
                                          dtype=torch.float32, device=self.device)

    @property
    def n_groups(self):
        """the groups of one pass over the loader"""
        return self._items()

    def form(self, idx, count=None, draw=0, window_ids=None):
        """One native call for explicit indices ``(K, G)`` and counts ``(G,)`` (None: K everywhere) -> ``GroupBatch``."""
        N, P = self._N, self.group_size
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.ndim != 2 or idx.shape[0] != self.K or not 1 <= idx.shape[1] <= self.batch_size:
            raise ValueError(f"need a ({self.K}, 1..{self.batch_size}) index array, got shape {idx.shape}")
        G = idx.shape[1]
        idx_dev = torch.from_numpy(idx).to(self.device, non_blocking=True)
        count_dev = None if count is None else torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(self.device, non_blocking=True)
        if count_dev is not None and count_dev.shape != (G,):
            raise ValueError(f"need {G} counts, got shape {tuple(count_dev.shape)}")
        ids_dev = None if window_ids is None else torch.as_tensor(np.ascontiguousarray(window_ids, dtype=np.int64)).to(self.device, non_blocking=True)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        tgt, cond, rest = new(P * G, self.RT, self.MZ), new(P * G, self.RT, self.MZ), new(G, self.RT, self.MZ)
        m1, w = new(P * G, *self.ms1_shape), new(G, self.K)
        import ctypes

        fixed = None if self.weights is None else (ctypes.c_float * self.K)(*self.weights)
        N.check(N.lib().dq_mix_group_batch(N.ptr(self.ms2), N.ptr(self.ms1), self.n, N.ptr(idx_dev), N.ptr(count_dev), G, self.K, P, self.RT,
                                           self.MZ, self.ms1_per, fixed, self.max_ratio_log2, N.ptr(self._seed_dev), N.ptr(ids_dev), int(draw),
                                           int(self.scale_target), N.ptr(tgt), N.ptr(m1), N.ptr(cond), N.ptr(rest), N.ptr(w),
                                           N.ptr(self._group_scratch), self._group_scratch.numel() * 4, N.stream_ptr()), "dq_mix_group_batch")
        return GroupBatch((tgt, m1, rest, None), cond, w, P)
