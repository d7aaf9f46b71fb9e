"""
The reference's segment tokenizer (`ecg_transformer/models/ecg_tokenizer.py`: `EcgPadder` :88-137, `EcgTokenizer` :140-626) on the device:
every lead is cut into k-sample segments, each segment loses its mean, the segments are clustered by k-means and a record is encoded as
(token id, segment mean) per segment.  The three sweeps over the data -- nearest centre, the Lloyd update, the decode -- are HIP kernels
(`csrc/tokenize.hip`) that read a resident record store in place; the host side here builds address tables, runs the Lloyd loop and keeps the
vocabulary.  There is no CPU fallback: host tensors raise.

k-means++ seeding (the reference's default `init`) is a kernel pair too: `EcgTokenizer.kmeans_plusplus`, and `init=KMeansPlusPlus()` in `fit`.

Scalable k-means++ (k-means||, Bahmani et al. 2012; what the reference's GPU backend asks cuML for as `init='scalable-k-means++'`) is
`EcgTokenizer.kmeans_parallel` and `init=ScalableKMeansPlusPlus()` in `fit` (`csrc/tok_scalable.hip`, include/ecgvit_hip_tok_scalable.h): a
few oversampling rounds over the store whatever the number of centres, then weighted k-means++ over the candidates.  It is the paper's
algorithm under this project's integer rules, not cuML's random stream or its exact variant: parity with cuML is UNPINNED (cuML is not
available to the tests), and the string stays refused.

DBSCAN (the reference's `dbscan` clustering) runs on the device as well (`csrc/dbscan.hip`): `EcgTokenizer.segments`, `EcgTokenizer.dbscan`, and
`method=Dbscan()` in `fit`.  Two all-pairs sweeps and a union-find over the core segments; the contract is in include/ecgvit_hip.h.

Not built: `save` / pickling, the plots and the three clusterings that are sequential by construction (DESIGN.md says why).
"""
import math
from ctypes import POINTER, c_uint64

import numpy as np
import torch

from . import hip, tok_scalable_abi
from .hip import lib, run, ptr, stream
from .records import DeviceTables, check_device_store, select_records

SEGMENT_SIZES = (8, 16, 32)
PADS = {'zero': 0, 'shift': 1}
MAX_CLUSTERS = hip.TOK_MAX_CLUSTERS
MAX_LOCAL_TRIALS = hip.TOK_MAX_LOCAL_TRIALS
MAX_ROUNDS = tok_scalable_abi.MAX_ROUNDS     # oversampling rounds of the scalable seeding (csrc/tok_scalable.hip)
SEED_SPAN = hip.TOK_SEED_SPAN        # consecutive positions of one lead per workgroup of the seeding's sweep (csrc/tokenize.hip)
DBSCAN_TILE = hip.TOK_DBSCAN_TILE    # segments per LDS tile of a DBSCAN sweep's column side (csrc/dbscan.hip)
DBSCAN_ROWS = {8: 1024, 16: 1024, 32: 512}      # rows per workgroup of a DBSCAN sweep, by k: 256 threads, four or two rows each
DBSCAN_PAIRS_PER_LAUNCH = 1 << 40               # no launch of a DBSCAN sweep covers more pairs (about a second of work): a sweep is enqueued as launches over row blocks
D_CLS_TH = dict(hierarchical='distance_threshold', dbscan='eps', optics='max_eps', birch='threshold', kmeans='n_clusters')   # ecg_tokenizer.py:72-78


class _Store(DeviceTables):
    """the device tables of one sweep: where every (record, lead) run starts, how long it is (`DeviceTables`), where its segments' outputs go"""

    def __init__(self, x, src_off, raw_len, stride, C, ragged, k, pad):
        check_device_store(x, 'signals')
        super().__init__(x, src_off, raw_len, stride)
        nseg = self.raw_len_h // k + 1                # a whole extra segment when k divides the length (EcgPadder never takes its n_pad == 0 branch)
        self.seg_cum = np.concatenate([[0], np.cumsum(nseg)]).astype(np.int64)
        self.k, self.pad, self.C, self.ragged = k, PADS[pad], int(C), ragged
        self.n_seg = int(self.seg_cum[-1])
        if ragged:
            dst_off, self.dst_stride, self.out_shape = self.seg_cum[:-1], self.n_seg, (self.C, self.n_seg)
        else:
            T = int(nseg[0])
            dst_off, self.dst_stride, self.out_shape = np.arange(self.R, dtype=np.int64) * (self.C * T), T, (self.R, self.C, T)
        self.seg_cum_d = torch.from_numpy(self.seg_cum).to(x.device)
        self.dst_off = torch.from_numpy(np.ascontiguousarray(dst_off, np.int64)).to(x.device)

    def args(self, x=None):
        return (ptr(self.x if x is None else x), ptr(self.src_off), self.stride, ptr(self.raw_len), ptr(self.seg_cum_d), ptr(self.dst_off),
                self.dst_stride, self.R, self.C, self.n_seg, self.k)

    def new(self, dtype):
        return torch.empty(self.out_shape, dtype=dtype, device=self.x.device)


def check_local_trials(n_local_trials):
    if n_local_trials is not None and not (isinstance(n_local_trials, (int, np.integer)) and 1 <= n_local_trials <= MAX_LOCAL_TRIALS):
        raise ValueError(f'n_local_trials = {n_local_trials!r}: None (2 + int(log(n_clusters))) or an int from 1 to {MAX_LOCAL_TRIALS}')
    return n_local_trials


class KMeansPlusPlus:
    """`fit(..., cls_kwargs=dict(init=KMeansPlusPlus(), ...))`: every restart is seeded on the device by `EcgTokenizer.kmeans_plusplus`'s kernels
    (sklearn's greedy k-means++; n_local_trials as there, None = 2 + int(log(n_clusters)), at most 16).  An object, not the string: the string
    `'k-means++'` promises sklearn's random stream as well, which the device does not reproduce, and stays refused."""

    def __init__(self, n_local_trials=None):
        self.n_local_trials = check_local_trials(n_local_trials)

    def __repr__(self):
        return f'{self.__class__.__qualname__}(n_local_trials={self.n_local_trials})'

    def trials(self, V):
        """the trials per centre for a table of V rows: sklearn's default rule, held to what the kernels take"""
        T = 2 + int(np.log(V)) if self.n_local_trials is None else int(self.n_local_trials)
        return min(T, MAX_LOCAL_TRIALS)


def check_oversampling(oversampling_factor, n_rounds):
    f = oversampling_factor
    if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or not np.isfinite(f) or not f > 0:
        raise ValueError(f'oversampling_factor = {f!r}: a finite positive number')
    if isinstance(n_rounds, bool) or not isinstance(n_rounds, (int, np.integer)) or not 1 <= n_rounds <= MAX_ROUNDS:
        raise ValueError(f'n_rounds = {n_rounds!r}: an int from 1 to {MAX_ROUNDS}')
    return float(f), int(n_rounds)


def scalable_cap(ell):
    """the most rows one round appends: ell + 8 ceil(sqrt(ell)), eight standard deviations past the expected ell"""
    return ell + 8 * (math.isqrt(ell - 1) + 1)


class ScalableKMeansPlusPlus:
    """`fit(..., cls_kwargs=dict(init=ScalableKMeansPlusPlus(), ...))`: every restart is seeded on the device by `EcgTokenizer.kmeans_parallel`'s
    kernels: scalable k-means++ (k-means||, Bahmani et al. 2012) -- n_rounds sweeps that each take a segment with probability
    min(1, ell q / pot), ell = ceil(oversampling_factor * n_clusters), then weighted greedy k-means++ over the candidates (n_local_trials as in
    `KMeansPlusPlus`).  The defaults are cuML's oversampling_factor and the paper's five rounds.  An object, not the string: it is the paper's
    algorithm under this project's integer rules, not cuML's random stream or its exact variant (parity with cuML is unpinned), and the
    string `'scalable-k-means++'` stays refused."""

    def __init__(self, oversampling_factor=2.0, n_rounds=5, n_local_trials=None):
        self.n_local_trials = check_local_trials(n_local_trials)
        self.oversampling_factor, self.n_rounds = check_oversampling(oversampling_factor, n_rounds)
        self._cap = None      # the tests' override of `scalable_cap`

    def __repr__(self):
        return (f'{self.__class__.__qualname__}(oversampling_factor={self.oversampling_factor}, n_rounds={self.n_rounds}, '
                f'n_local_trials={self.n_local_trials})')

    trials = KMeansPlusPlus.trials

    def plan(self, V):
        """-> (T, R, ell, cap) for a table of V rows; the candidate table of 1 + R cap rows is held to the largest table here, on the host"""
        ell = max(1, math.ceil(self.oversampling_factor * V))
        cap = scalable_cap(ell) if self._cap is None else int(self._cap)
        if cap < 1 or ell > MAX_CLUSTERS or 1 + self.n_rounds * cap > MAX_CLUSTERS:
            raise ValueError(f'n_clusters = {V}, oversampling_factor = {self.oversampling_factor}, n_rounds = {self.n_rounds}: ell = {ell} segments '
                             f'expected and at most {cap} appended per round make a candidate table of up to {1 + self.n_rounds * cap} rows; '
                             f'a table holds at most {MAX_CLUSTERS}')
        return self.trials(V), self.n_rounds, ell, cap


def check_min_samples(min_samples):
    if not (isinstance(min_samples, (int, np.integer)) and not isinstance(min_samples, bool) and min_samples >= 1):
        raise ValueError(f'min_samples = {min_samples!r}: an int, at least 1')
    return int(min_samples)


def check_eps(eps):
    """-> eps2 = fl32(fl32(eps) * fl32(eps)), what the kernels compare against"""
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not np.isfinite(eps) or not eps > 0:
        raise ValueError(f'eps = {eps!r}: a finite positive number')
    e = np.float32(eps)
    with np.errstate(over='ignore'):
        eps2 = np.float32(e * e)
    if not np.isfinite(eps2):
        raise ValueError(f'eps = {eps!r}: its square is not a finite float32')
    return float(eps2)


class Dbscan:
    """`fit(..., method=Dbscan(), cls_kwargs=dict(eps=...))`: sklearn's DBSCAN over the mean-removed segments, on the device
    (`EcgTokenizer.dbscan`); min_samples as the reference's `cluster_args` has it, `cls_kwargs['min_samples']` overrides it.  An object, not
    the string: the string `'dbscan'` promises sklearn's f64 comparison at eps as well, which the f32 kernels do not reproduce for a pair
    within rounding of eps, and stays refused."""

    def __init__(self, min_samples=5):
        self.min_samples = check_min_samples(min_samples)

    def __repr__(self):
        return f'{self.__class__.__qualname__}(min_samples={self.min_samples})'


def check_lengths(lengths, k, pad):
    """the one place run lengths are held to the padder's rule: 'shift' copies the n_pad = k - l % k samples before the end, so needs l >= n_pad"""
    lengths = np.asarray(lengths, np.int64)
    if lengths.size == 0 or int(lengths.min()) < 1:
        raise ValueError('every record needs at least one sample')
    if pad == 'shift':
        bad = lengths < k - lengths % k
        if bad.any():
            l = int(lengths[bad][0])
            raise ValueError(f"pad='shift' copies the last n_pad = k - l % k samples: l = {l} is shorter than n_pad = {k - l % k} (use pad='zero')")
    return lengths


class EcgTokenizer:
    """`EcgTokenizer(k=8, pad='shift')`: `centers` (V, k) f32 and `lens` (V,) int64 numpy arrays, `fit_method`, `n_sig`, `cls_th` as the
    reference sets them.  Signals are float32 device tensors: (…, C, L), or a ragged (12, S_total) store with `offsets`."""

    def __init__(self, k=2 ** 3, pad='shift'):
        if k not in SEGMENT_SIZES:
            raise ValueError(f'k = {k}: the kernels are built for k in {SEGMENT_SIZES}')
        if pad not in PADS:
            raise ValueError(f"pad = {pad!r}: one of 'zero', 'shift'")
        self.k, self.pad = k, pad
        self._tables = {}     # (device, th) -> the device copy of the (cut) table
        self._cut = {}        # th -> host rows kept (the reference's CustNN.data)
        self.centers = self.lens = None
        self.fit_method = self.n_sig = self.cls_th = None
        self.n_iter_ = self.inertia_ = self.changed_ = None     # of the last fit: assign passes run, sum of dist, ids changed per pass
        self.n_noise = self.labels_ = None                      # of the last DBSCAN fit: segments left out as noise, every segment's label (-1: noise)

    # the vocabulary: assigning either array drops every table derived from the old one (device copies, th cuts)
    @property
    def centers(self):
        return self._centers

    @centers.setter
    def centers(self, v):
        self._centers = v
        self._tables.clear()
        self._cut.clear()

    @property
    def lens(self):
        return self._lens

    @lens.setter
    def lens(self, v):
        self._lens = v
        self._tables.clear()
        self._cut.clear()

    def __repr__(self):
        return f'<{self.__class__.__qualname__} k={self.k} pad={self.pad}>'

    def n_segments(self, l):
        """segments of a run of l samples: l // k + 1 (16 samples at k = 8 pad to 24)"""
        return int(l) // self.k + 1

    @classmethod
    def from_centers(cls, centers, lens, pad='shift'):
        """a vocabulary fitted elsewhere: centers (V, k), lens (V,) cluster sizes"""
        centers = np.ascontiguousarray(centers.detach().cpu().numpy() if isinstance(centers, torch.Tensor) else centers, dtype=np.float32)
        lens = np.asarray(lens.detach().cpu().numpy() if isinstance(lens, torch.Tensor) else lens).astype(np.int64)
        if centers.ndim != 2 or lens.shape != (centers.shape[0],):
            raise ValueError(f'centers must be (V, k) and lens (V,), got {centers.shape} and {lens.shape}')
        if not 1 <= centers.shape[0] <= MAX_CLUSTERS:
            raise ValueError(f'{centers.shape[0]} centres: 1 to {MAX_CLUSTERS} are supported')
        tok = cls(k=centers.shape[1], pad=pad)
        tok.centers, tok.lens = centers, lens
        return tok

    # ---- the table ----------------------------------------------------------------------------------
    def _rows(self, th):
        """host rows of the table under threshold `th`: the reference's CustNN (:193-220).  An int is an absolute lower bound on the cluster
        size.  For a float in (0, 1) the reference computes round(lens.sum() * th) but then compares `lens >= th` against the RAW fraction,
        which keeps every non-empty cluster: that quirk is kept."""
        if self.centers is None:
            raise RuntimeError('the tokenizer has no vocabulary: call fit() or from_centers()')
        if th is None:
            return self.centers
        if th not in self._cut:
            if not isinstance(th, (int, np.integer)) and not (isinstance(th, float) and 0 < th < 1):
                raise ValueError(f'th = {th!r}: an int, or a float in (0, 1)')
            rows = np.ascontiguousarray(self.centers[self.lens >= th])
            if len(rows) == 0:
                raise ValueError(f'th = {th} removes every centre')
            self._cut[th] = rows
        return self._cut[th]

    def _table(self, device, th):
        key = (str(device), th)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self._rows(th)).to(device)
        return self._tables[key]

    # ---- stores -------------------------------------------------------------------------------------
    def _dense_store(self, sig):
        """(…, L): every row is a run of its own (one lead per 'record'), so any number of leading dimensions serves"""
        if not isinstance(sig, torch.Tensor) or sig.dim() < 1:
            raise ValueError('signals must be a float32 device tensor of shape (…, C, L)')
        L = int(sig.shape[-1])
        check_lengths([L], self.k, self.pad)
        rows = int(np.prod(sig.shape[:-1], dtype=np.int64))
        if rows < 1:
            raise ValueError('no signal given')
        return _Store(sig, np.arange(rows, dtype=np.int64) * L, np.full(rows, L, np.int64), L, 1, False, self.k, self.pad)

    def _record_store(self, sigs, offsets, idxs, n_clusters=None):
        """(n, 12, L) records or a ragged (12, S_total) store with offsets, and a subset of either: the convention and validator of `records.py`.
        n_clusters: held against the segment count (a seeding chooses that many segments), before a device is asked for"""
        if not isinstance(sigs, torch.Tensor):
            raise ValueError('signals must be a float32 device tensor (no CPU fallback exists)')
        s = select_records(sigs, offsets, idxs)
        check_lengths(s.raw_len, self.k, self.pad)
        if n_clusters is not None and n_clusters > s.C * int((s.raw_len // self.k + 1).sum()):
            raise ValueError(f'n_clusters = {n_clusters} exceeds the {s.C * int((s.raw_len // self.k + 1).sum())} segments of the store')
        return _Store(sigs, s.src_off, s.raw_len, s.stride, s.C, not s.rect, self.k, self.pad)

    # ---- kernels ------------------------------------------------------------------------------------
    def _assign(self, st, table, ids, means, dist=None, prev_ids=None, changed=None):
        run.ecgvit_tok_assign(*st.args(), st.pad, ptr(table), table.shape[0], ptr(prev_ids), ptr(ids), ptr(means), ptr(dist), ptr(changed),
                              stream())

    def _update(self, st, ids, table, lens, ws, keep_amax=False):
        """keep_amax: `ws` was last used by an update over this very store, whose absolute maximum it still holds: that sweep is skipped"""
        run.ecgvit_tok_update(*st.args(), st.pad, ptr(ids), ptr(table), table.shape[0], ptr(lens), ptr(ws), int(keep_amax), stream())

    def _seed(self, st, V, T, first, u53, trace=False, ws=None, keep_amax=False):
        """one k-means++ seeding, enqueued whole: -> (centres (V, k) f32, indices (V,) int64 [g = c * n_seg + p], trace (V - 1, T, 2) int64 or
        None, the workspace), device tensors.  u53: (V - 1, T) uint64 host array, floor(u 2^53).  keep_amax: `ws` comes from a seeding over this
        very store, whose absolute maximum it still holds"""
        dev = st.x.device
        nbytes = lib().ecgvit_tok_seed_workspace(st.C, st.n_seg, V, st.k, T)
        if nbytes == 0:
            raise ValueError(f'a seeding of {V} centres with {T} trials over {st.C} x {st.n_seg} segments is not supported (1 to {MAX_LOCAL_TRIALS} '
                             f'trials, n_clusters at most the segment count, fewer than 2^32 segments)')
        if ws is None:
            ws, keep_amax = torch.empty(nbytes // 8, dtype=torch.int64, device=dev), False
        u53 = np.ascontiguousarray(u53, np.uint64).reshape(V - 1, T)
        if u53.size and int(u53.max()) >= 2 ** 53:
            raise ValueError('u53 holds floor(u 2^53) of uniform draws u in [0, 1)')
        u_d = torch.from_numpy(u53.view(np.int64).reshape(-1).copy()).to(dev) if u53.size else None
        centers = torch.empty((V, st.k), dtype=torch.float32, device=dev)
        indices = torch.empty(V, dtype=torch.int64, device=dev)
        tr = torch.zeros((V - 1, T, 2), dtype=torch.int64, device=dev) if trace else None
        run.ecgvit_tok_seed(*st.args(), st.pad, V, T, int(first), ptr(u_d), ptr(centers), ptr(indices), ptr(tr), ptr(ws), int(keep_amax),
                            stream())
        return centers, indices, tr, ws

    @staticmethod
    def _seed_draws(rng, total, V, T):
        """what one seeding takes from the generator, in this order: the first centre, then a (V - 1, T) block of uniforms"""
        first = int(rng.integers(total))
        return first, np.floor(rng.random((V - 1, T)) * 2.0 ** 53).astype(np.uint64)

    def _seed_scalable(self, st, V, T, R, ell, cap, first, keys, u0, u53, ws=None, keep_amax=False):
        """one scalable seeding, enqueued whole: -> (centres (V, k) f32, indices (V,) int64, cand_g and weights (1 + R cap,) int64, info, the
        workspace), device tensors; only the first info[0] = n_c candidates count, and centres / indices are written only when n_c >= V (the
        caller reads `info`).  keys: (R,) uint64 and u0 < 2^53 on the host; u53: (V - 1, T) uint64 host array"""
        dev = st.x.device
        nbytes = tok_scalable_abi.lib().ecgvit_tok_scalable_workspace(st.C, st.n_seg, V, st.k, T, R, cap)
        if nbytes == 0:
            raise ValueError(f'a scalable seeding of {V} centres with {T} trials, {R} rounds of at most {cap} rows over {st.C} x {st.n_seg} segments '
                             f'is not supported (1 to {MAX_LOCAL_TRIALS} trials, 1 to {MAX_ROUNDS} rounds, at most {MAX_CLUSTERS} candidate rows, '
                             f'n_clusters at most the segment count, fewer than 2^32 segments)')
        if ws is None:
            ws, keep_amax = torch.empty(nbytes // 8, dtype=torch.int64, device=dev), False
        u53 = np.ascontiguousarray(u53, np.uint64).reshape(V - 1, T)
        keys = np.ascontiguousarray(keys, np.uint64).reshape(R)
        if (u53.size and int(u53.max()) >= 2 ** 53) or not 0 <= int(u0) < 2 ** 53:
            raise ValueError('u0 and u53 hold floor(u 2^53) of uniform draws u in [0, 1)')
        u_d = torch.from_numpy(u53.view(np.int64).reshape(-1).copy()).to(dev) if u53.size else None
        rows = 1 + R * cap
        centers = torch.zeros((V, st.k), dtype=torch.float32, device=dev)
        indices = torch.zeros(V, dtype=torch.int64, device=dev)
        cand_g = torch.zeros(rows, dtype=torch.int64, device=dev)
        weights = torch.empty(rows, dtype=torch.int64, device=dev)
        info = torch.empty(tok_scalable_abi.info_words(R), dtype=torch.int64, device=dev)
        tok_scalable_abi.run.ecgvit_tok_scalable_seed(*st.args(), st.pad, V, T, R, ell, cap, int(first), keys.ctypes.data_as(POINTER(c_uint64)),
                                                      int(u0), ptr(u_d), ptr(centers), ptr(indices), ptr(cand_g), ptr(weights), ptr(info), ptr(ws),
                                                      int(keep_amax), stream())
        return centers, indices, cand_g, weights, info, ws

    @staticmethod
    def _scalable_draws(rng, total, V, T, R):
        """what one scalable seeding takes from the generator, in this order: the first candidate, the R round keys, u0, then a (V - 1, T) block
        of uniforms"""
        first = int(rng.integers(total))
        keys = rng.integers(0, 2 ** 64, size=R, dtype=np.uint64)
        u0 = int(np.floor(rng.random() * 2.0 ** 53))
        return first, keys, u0, np.floor(rng.random((V - 1, T)) * 2.0 ** 53).astype(np.uint64)

    @staticmethod
    def _scalable_info(info, init, V):
        """the one small read of a scalable seeding -> (n_c, selected (R,), truncated (R,), pots (R + 1,) uint64); too few candidates raise"""
        h = info.cpu().numpy().view(np.uint64)
        R, H = init.n_rounds, tok_scalable_abi.INFO_HEAD
        n_c = int(h[0])
        if n_c < V:
            raise ValueError(f'the scalable seeding ended with n_c = {n_c} candidates, fewer than n_clusters = {V}: raise n_rounds = {R} or '
                             f'oversampling_factor = {init.oversampling_factor} (a store with fewer than {V} distinct segments has no such seeding)')
        return n_c, h[H:H + R].astype(np.int64), h[H + R:H + 2 * R].astype(np.int64), h[H + 2 * R:H + 3 * R + 1].copy()

    def kmeans_parallel(self, sigs, n_clusters, random_state=None, oversampling_factor=2.0, n_rounds=5, n_local_trials=None, offsets=None,
                        idxs=None, return_info=False, _cap=None):
        """Scalable k-means++ (k-means||, Bahmani et al. 2012) over the mean-removed segments of a store `fit` takes -> (centers (V, k) f32,
        indices (V,) int64), numpy arrays, as `kmeans_plusplus` returns them.  n_rounds sweeps whatever V is: each round takes segment g with
        probability min(1, ell q(g) / pot), ell = ceil(oversampling_factor * V), from a counter-based generator keyed per round; the candidates
        are weighted by the segments nearest to them and reclustered by weighted greedy k-means++ (n_local_trials as in `kmeans_plusplus`).
        The contract, every integer rule included: include/ecgvit_hip_tok_scalable.h.  It is the paper's algorithm, not cuML's random stream
        or its exact variant: parity with the reference's cuML backend is unpinned.
        `random_state` seeds `np.random.default_rng` (a Generator is used as it is), which gives, in this order: the first candidate, the
        n_rounds keys (uint64), u0 for the first centre, then (V - 1, n_local_trials) uniforms.
        return_info: also a dict -- cand_g (n_c,) the candidates' segments in table order, weights (n_c,), selected / truncated (n_rounds,) the
        segments each round's rule took and how many of them the per-round cap dropped, pots (n_rounds,) uint64 the potential each round drew
        under, potential: the one after the last fold.  Fewer candidates than n_clusters is a ValueError."""
        V = int(n_clusters)
        if not 1 <= V <= MAX_CLUSTERS:
            raise ValueError(f'n_clusters = {V}: 1 to {MAX_CLUSTERS} are supported')
        init = ScalableKMeansPlusPlus(oversampling_factor, n_rounds, n_local_trials)
        init._cap = _cap
        T, R, ell, cap = init.plan(V)
        st = self._record_store(sigs, offsets, idxs, n_clusters=V)
        rng = np.random.default_rng(random_state)
        with torch.cuda.device(sigs.device):
            first, keys, u0, u53 = self._scalable_draws(rng, st.C * st.n_seg, V, T, R)
            centers, indices, cand_g, weights, info, _ = self._seed_scalable(st, V, T, R, ell, cap, first, keys, u0, u53)
            n_c, selected, truncated, pots = self._scalable_info(info, init, V)
            out = centers.cpu().numpy(), indices.cpu().numpy()
            if return_info:
                out += (dict(cand_g=cand_g[:n_c].cpu().numpy(), weights=weights[:n_c].cpu().numpy(), selected=selected, truncated=truncated,
                             pots=pots[:R], potential=int(pots[R])),)
            return out

    def kmeans_plusplus(self, sigs, n_clusters, random_state=None, n_local_trials=None, offsets=None, idxs=None):
        """`sklearn.cluster.kmeans_plusplus` over the mean-removed segments of a store `fit` takes -> (centers (V, k) f32, indices (V,) int64),
        numpy arrays; index g = c * n_seg + p is segment p of lead c, counted over the selected records in order.  sklearn's greedy algorithm
        (n_local_trials candidates per centre, drawn in proportion to the squared distance to the nearest chosen centre; the one that leaves
        the smallest potential is kept) with integer sums (include/ecgvit_hip.h), not sklearn's random stream: `random_state` seeds
        `np.random.default_rng` (a Generator is used as it is), which gives the first centre and then (V - 1, n_local_trials) uniforms."""
        V = int(n_clusters)
        if not 1 <= V <= MAX_CLUSTERS:
            raise ValueError(f'n_clusters = {V}: 1 to {MAX_CLUSTERS} are supported')
        T = KMeansPlusPlus(n_local_trials).trials(V)
        st = self._record_store(sigs, offsets, idxs, n_clusters=V)
        rng = np.random.default_rng(random_state)
        with torch.cuda.device(sigs.device):
            first, u53 = self._seed_draws(rng, st.C * st.n_seg, V, T)
            centers, indices, _, _ = self._seed(st, V, T, first, u53)
            return centers.cpu().numpy(), indices.cpu().numpy()

    # ---- DBSCAN -------------------------------------------------------------------------------------
    def _segment_store(self, sigs, offsets, idxs):
        """the store of a DBSCAN pass; the segment count is held to the sweeps' int32 indices before a device is asked for"""
        if isinstance(sigs, torch.Tensor):
            s = select_records(sigs, offsets, idxs)
            n = s.C * int((s.raw_len // self.k + 1).sum())
            if n >= 2 ** 31:
                raise ValueError(f'{n} segments: the pair sweeps index fewer than 2^31')
        return self._record_store(sigs, offsets, idxs)

    def _segments(self, st, want_dst=False):
        """-> (segs (n, k) f32, means (n,) f32, dst (n,) int64 or None): the dense table in the reference's flat order; dst: where segment q
        has its id in a tensor of `st.out_shape`"""
        dev, n = st.x.device, st.C * st.n_seg
        segs = torch.empty((n, self.k), dtype=torch.float32, device=dev)
        means = torch.empty(n, dtype=torch.float32, device=dev)
        dst = torch.empty(n, dtype=torch.int64, device=dev) if want_dst else None
        run.ecgvit_tok_segments(*st.args(), st.pad, ptr(segs), ptr(means), ptr(dst), stream())
        return segs, means, dst

    def segments(self, sigs, offsets=None, idxs=None):
        """-> (segs (n, k) f32, means (n,) f32), device tensors: the mean-removed segments of a store `fit` takes and their means, in the
        reference's flat order `sigs.reshape(-1, k)`: segment s of lead c of the r-th selected record is row 12 * (segments of the records
        before it) + c * n_r + s, whatever the store form.  The dense table every DBSCAN pass reads."""
        st = self._segment_store(sigs, offsets, idxs)
        with torch.cuda.device(sigs.device):
            return self._segments(st)[:2]

    def _row_blocks(self, rows, cols):
        """[row0, row1) per launch of a sweep of `rows` rows against `cols` columns: whole workgroups, at most DBSCAN_PAIRS_PER_LAUNCH pairs
        (one workgroup's rows where even that is more)"""
        rpb = DBSCAN_ROWS[self.k]
        step = max(1, DBSCAN_PAIRS_PER_LAUNCH // max(1, cols) // rpb) * rpb
        return [(lo, min(lo + step, rows)) for lo in range(0, rows, step)]

    def _dbscan(self, segs, eps2, min_samples):
        """the passes over a dense (n, k) table -> (core (m,) int64 ascending, labels (n,) int32, roots (m,) int32 or None), device tensors.
        torch compacts the core and the non-core rows and ranks the roots between the sweeps: plumbing; two host reads (the two counts)."""
        s, k, (n, dev) = stream(), self.k, (segs.shape[0], segs.device)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        for lo, hi in self._row_blocks(n, n):
            run.ecgvit_tok_dbscan_count(ptr(segs), n, k, eps2, lo, hi, ptr(count), s)
        is_core = count >= min_samples
        core = is_core.nonzero().view(-1)                 # ascending q
        labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
        m = int(core.numel())
        if m == 0:
            return core, labels, None
        table = segs.index_select(0, core)
        parent = torch.arange(m, dtype=torch.int32, device=dev)
        for lo, hi in self._row_blocks(m, m):
            if hi > 1:                                    # (row 0 has no column below it)
                run.ecgvit_tok_dbscan_link(ptr(table), m, k, eps2, lo, hi, ptr(parent), s)
        roots = torch.empty(m, dtype=torch.int32, device=dev)
        run.ecgvit_tok_dbscan_flatten(ptr(parent), m, ptr(roots), s)
        core_label = torch.unique(roots, sorted=True, return_inverse=True)[1].to(torch.int32)      # ascending root = ascending smallest q
        labels[core] = core_label
        rest = (~is_core).nonzero().view(-1)
        nb = int(rest.numel())
        if nb:
            rows = segs.index_select(0, rest)
            got = torch.empty(nb, dtype=torch.int32, device=dev)
            for lo, hi in self._row_blocks(nb, m):
                run.ecgvit_tok_dbscan_border(ptr(rows), nb, ptr(table), ptr(core_label), m, k, eps2, lo, hi, ptr(got), s)
            labels[rest] = got
        return core, labels, roots

    def dbscan(self, sigs, eps, min_samples=5, offsets=None, idxs=None):
        """`sklearn.cluster.dbscan` over the mean-removed segments of a store `fit` takes -> (core_sample_indices, labels), numpy int64 arrays
        in the flat order of `segments`; -1 is noise.  sklearn's algorithm and its labels (clusters numbered by their first core segment, a
        border segment with the first cluster that reaches it) with the f32 neighbour rule of include/ecgvit_hip.h: d2 <= fl32(eps)^2 on the
        unfused f32 chain, which differs from sklearn's f64 comparison only for a pair within (k + 2) 2^-24 of eps.  A segment with a
        non-finite sample is noise (sklearn raises)."""
        eps2, min_samples = check_eps(eps), check_min_samples(min_samples)
        st = self._segment_store(sigs, offsets, idxs)
        with torch.cuda.device(sigs.device):
            core, labels, _ = self._dbscan(self._segments(st)[0], eps2, min_samples)
            return core.cpu().numpy(), labels.cpu().numpy().astype(np.int64)

    def _fit_dbscan(self, sigs, method, cls_kwargs, offsets, idxs):
        """the reference's post-processing of a clustering with outliers (:413-422, :489-490): noise is dropped, `lens` are the cluster sizes
        (border members included) and `centers` the member means, through the Lloyd update's kernels (an id of -1 is left out there)"""
        kw = dict(min_samples=method.min_samples)
        kw.update(cls_kwargs or {})
        unknown = set(kw) - {'eps', 'min_samples'}
        if unknown:
            raise ValueError(f'cls_kwargs {sorted(unknown)} are not supported: eps, min_samples')
        if 'eps' not in kw:
            raise ValueError("cls_kwargs needs 'eps'")
        eps2, min_samples = check_eps(kw['eps']), check_min_samples(kw['min_samples'])
        st = self._segment_store(sigs, offsets, idxs)
        with torch.cuda.device(sigs.device):
            segs, _, dst = self._segments(st, want_dst=True)
            core, labels, roots = self._dbscan(segs, eps2, min_samples)
            n_noise = int((labels < 0).sum())
            V = 0 if roots is None else int(labels.max()) + 1
            if V == 0:
                raise ValueError(f"eps = {kw['eps']!r}, min_samples = {min_samples}: no cluster at all, every one of the {n_noise} segments is noise")
            if V > MAX_CLUSTERS:
                raise ValueError(f'{V} clusters: a vocabulary holds at most {MAX_CLUSTERS} (dbscan() still returns such labels)')
            ids = st.new(torch.int32)
            ids.view(-1)[dst] = labels
            table = torch.zeros((V, self.k), dtype=torch.float32, device=sigs.device)      # every cluster holds a core segment: every row is written
            lens = torch.zeros(V, dtype=torch.int64, device=sigs.device)
            ws = torch.empty(lib().ecgvit_tok_workspace(V, self.k) // 8, dtype=torch.int64, device=sigs.device)
            self._update(st, ids, table, lens, ws)
        self.fit_method, self.n_sig, self.cls_th = 'dbscan', st.R, kw['eps']
        self.n_iter_ = self.inertia_ = self.changed_ = None
        self.n_noise, self.labels_ = n_noise, ids
        self.centers, self.lens = table.cpu().numpy(), lens.cpu().numpy()
        return self

    # ---- encode / decode ----------------------------------------------------------------------------
    def __call__(self, sig, th=None, offsets=None):
        """-> (ids, means): for (…, C, L) input both of shape (…, C, L // k + 1); for a ragged (12, S_total) store with `offsets` both (12, T_total)
        and, third, `seg_offsets` ((n + 1,) int64: record r's segments are columns seg_offsets[r] : seg_offsets[r + 1]).  ids are int32 and means
        float32 (the reference returns int64 / float64).  The caller's signal is NOT modified (the reference's `segs -= means` writes through a
        view of it).  th: the reference's size threshold (`_rows`); ids then index the cut table, as `decode(ids, th)` reads them."""
        if offsets is None:
            st = self._dense_store(sig)
            shape = tuple(sig.shape[:-1]) + (st.out_shape[-1],)
        else:
            st = self._record_store(sig, offsets, None)
            shape = st.out_shape
        with torch.cuda.device(sig.device):
            table = self._table(sig.device, th)
            ids, means = st.new(torch.int32), st.new(torch.float32)
            self._assign(st, table, ids, means)
        if offsets is None:
            return ids.view(shape), means.view(shape)
        return ids, means, torch.from_numpy(st.seg_cum.copy())

    def decode(self, ids, th=None):
        """centers[ids] (…, k): the reference's decode (:346-350); with `th`, rows of the cut table"""
        if isinstance(ids, torch.Tensor):
            if ids.is_cuda:
                return self._table(ids.device, th)[ids.long()]
            ids = ids.numpy()
        return self._rows(th)[ids]

    def reconstruct(self, ids, means, lengths, th=None):
        """centers[ids] + means, cut to each run's length: what the reference plots beside the signal (:292).  lengths: an int L for
        (…, C, T) ids -> (…, C, L); a (n,) array of record lengths for the (12, T_total) ids of a ragged store -> (12, S_total)."""
        if not (isinstance(ids, torch.Tensor) and ids.is_cuda and isinstance(means, torch.Tensor) and means.is_cuda):
            raise ValueError('ids and means must be device tensors (no CPU fallback exists)')
        if ids.dtype != torch.int32 or means.dtype != torch.float32 or ids.shape != means.shape:
            raise ValueError('ids (int32) and means (float32) must have one shape, as __call__ returns them')
        ids, means = ids.contiguous(), means.contiguous()
        dev = ids.device
        if np.ndim(lengths) == 0:
            L = int(lengths)
            if ids.dim() < 1 or ids.shape[-1] != self.n_segments(L):
                raise ValueError(f'{ids.shape[-1] if ids.dim() else 0} segments per run do not belong to runs of {L} samples at k = {self.k}')
            out = torch.empty(tuple(ids.shape[:-1]) + (L,), dtype=torch.float32, device=dev)
            st = self._dense_store(out)
        else:
            lengths = check_lengths(lengths, self.k, 'zero')
            off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
            if ids.dim() != 2 or ids.shape[1] != int((lengths // self.k + 1).sum()):
                raise ValueError('ids must be (12, T_total) with T_total the segments of the given lengths')
            out = torch.empty((ids.shape[0], int(off[-1])), dtype=torch.float32, device=dev)
            st = self._record_store(out, off, None)
        with torch.cuda.device(dev):
            table = self._table(dev, th)
            run.ecgvit_tok_decode(*st.args(), ptr(ids), ptr(means), ptr(table), table.shape[0], stream())
        return out

    # ---- fit ----------------------------------------------------------------------------------------
    def _random_init(self, st, V, rng):
        """V distinct segments of the store, mean removed, drawn by a seeded host generator"""
        total = st.C * st.n_seg
        if V > total:
            raise ValueError(f'n_clusters = {V} exceeds the {total} segments of the store')
        pick = rng.choice(total, size=V, replace=False)
        c, p = pick // st.n_seg, pick % st.n_seg
        r = np.searchsorted(st.seg_cum, p, side='right') - 1
        l = st.raw_len_h[r][:, None]
        i = ((p - st.seg_cum[r]) * self.k)[:, None] + np.arange(self.k)[None, :]
        n_pad = self.k - l % self.k
        keep = (i < l) | (st.pad == 1)
        i = np.where(i < l, i, np.clip(i - n_pad, 0, l - 1))
        flat = st.src_off_h[r][:, None] + c[:, None] * st.stride + i
        dev = st.x.device
        seg = st.x.reshape(-1)[torch.from_numpy(flat).to(dev)]
        seg = torch.where(torch.from_numpy(keep).to(dev), seg, torch.zeros_like(seg))      # (a select: a NaN at the clamped index stays out)
        return (seg - seg.mean(dim=1, keepdim=True)).contiguous()

    def _lloyd(self, st, table, max_iter, ws, ws_state):
        """-> (centres, lens, inertia, ids changed per assign).  Every assign also writes `dist`, so no pass is spent on the inertia.  A run that
        converges ends on an assign that changed nothing: ids, dist, centres and lens all belong together.  A run that ends at max_iter ends on
        an update: centres and lens are the means and the counts of the last assign's labels -- how the reference builds them from `labels_`
        (:489-490) -- and the inertia is that assign's, taken under the centres before the last update (an upper bound of the final one)."""
        dev = st.x.device
        ids, means, dist = st.new(torch.int32).fill_(-1), st.new(torch.float32), st.new(torch.float32)
        changed = torch.zeros(1, dtype=torch.int64, device=dev)
        lens = torch.zeros(table.shape[0], dtype=torch.int64, device=dev)
        history = []
        for _ in range(max_iter):
            self._assign(st, table, ids, means, dist=dist, prev_ids=ids, changed=changed)
            history.append(int(changed.item()))     # the iteration's one sync: 8 bytes
            if history[-1] == 0:
                break                               # the centres already are the means of these ids
            self._update(st, ids, table, lens, ws, keep_amax=ws_state['amax'])     # the store's absolute maximum is swept once per fit
            ws_state['amax'] = True
        return table, lens, float(dist.sum(dtype=torch.float64)), history

    def fit(self, sigs, method='kmeans', cls_kwargs=None, offsets=None, idxs=None):
        """k-means over the mean-removed segments of `sigs`: (n, 12, L) float32 device records, or a ragged (12, S_total) store with `offsets`;
        `idxs` selects records without a copy (the record-store convention of `records.py`).
        cls_kwargs: n_clusters (required), max_iter=256, n_init=1, random_state=None, init='random' (n_clusters distinct segments drawn by a
        seeded host generator), a `KMeansPlusPlus()` object (every restart seeded on the device, `kmeans_plusplus`; with n_init=8 the
        reference's default configuration), a `ScalableKMeansPlusPlus()` object (every restart seeded on the device by `kmeans_parallel`: a few
        sweeps whatever n_clusters is; the algorithm the reference's cuML backend names, parity with cuML unpinned) or a (n_clusters, k) array (Lloyd from a given start is deterministic).  Lloyd iterations are assign then update;
        they stop when an iteration changes no id, or at max_iter; n_init > 1 keeps the run of lowest inertia.  A centre that loses every
        segment keeps its value with size 0.  Label order is the clustering's own, as in the reference; nothing is reordered.
        method=Dbscan(min_samples=5) with cls_kwargs=dict(eps=..., min_samples=...): DBSCAN instead (`dbscan`), with the reference's
        post-processing: noise is dropped (`n_noise`), `lens` are the cluster sizes, `centers` the member means, `labels_` every segment's label
        (int32, device, -1: noise) in the layout of the ids `tok(sig)` returns; no cluster at all, or more than MAX_CLUSTERS, is a ValueError."""
        if isinstance(method, Dbscan):
            return self._fit_dbscan(sigs, method, cls_kwargs, offsets, idxs)
        if method != 'kmeans':
            if method in D_CLS_TH:
                raise NotImplementedError(f"method = {method!r}: only 'kmeans' runs on the device (the hierarchical and density methods are not data-parallel in this form)")
            raise ValueError(f'method = {method!r}: one of {sorted(D_CLS_TH)}')
        kw = dict(max_iter=256, n_init=1, random_state=None, init='random')
        kw.update(cls_kwargs or {})
        unknown = set(kw) - {'n_clusters', 'max_iter', 'n_init', 'random_state', 'init'}
        if unknown:
            raise ValueError(f'cls_kwargs {sorted(unknown)} are not supported: n_clusters, max_iter, n_init, random_state, init')
        if 'n_clusters' not in kw:
            raise ValueError("cls_kwargs needs 'n_clusters'")
        V, max_iter, n_init, init = int(kw['n_clusters']), int(kw['max_iter']), int(kw['n_init']), kw['init']
        if not 1 <= V <= MAX_CLUSTERS:
            raise ValueError(f'n_clusters = {V}: 1 to {MAX_CLUSTERS} are supported')
        if max_iter < 1 or n_init < 1:
            raise ValueError('max_iter and n_init must be at least 1')
        fixed = plus = scalable = None
        if isinstance(init, str):
            if init != 'random':
                raise NotImplementedError(f"init = {init!r}: 'random', a KMeansPlusPlus() object (k-means++ seeding on the device: sklearn's algorithm, "
                                          f"not the random stream the string promises) or a (n_clusters, k) array are supported")
        elif isinstance(init, ScalableKMeansPlusPlus):
            scalable = init.plan(V)
        elif isinstance(init, KMeansPlusPlus):
            plus = init.trials(V)
        else:
            fixed = np.ascontiguousarray(init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else init, dtype=np.float32)
            if fixed.shape != (V, self.k):
                raise ValueError(f'init must be ({V}, {self.k}), got {fixed.shape}')
        st = self._record_store(sigs, offsets, idxs, n_clusters=V if plus or scalable else None)
        rng = np.random.default_rng(kw['random_state'])
        best = seed_ws = None
        with torch.cuda.device(sigs.device):
            ws = torch.empty(lib().ecgvit_tok_workspace(V, self.k) // 8, dtype=torch.int64, device=sigs.device)
            ws_state = dict(amax=False)
            for _ in range(1 if fixed is not None else n_init):
                if plus:                # the table stays on the device; the seeding's sweep for the absolute maximum serves every update too
                    first, u53 = self._seed_draws(rng, st.C * st.n_seg, V, plus)
                    table, _, _, seed_ws = self._seed(st, V, plus, first, u53, ws=seed_ws, keep_amax=seed_ws is not None)
                elif scalable:          # the same sharing: both seedings keep the maximum in the first 16 bytes of their workspace
                    T, R, ell, cap = scalable
                    first, keys, u0, u53 = self._scalable_draws(rng, st.C * st.n_seg, V, T, R)
                    table, _, _, _, info, seed_ws = self._seed_scalable(st, V, T, R, ell, cap, first, keys, u0, u53, ws=seed_ws,
                                                                        keep_amax=seed_ws is not None)
                    self._scalable_info(info, init, V)
                if (plus or scalable) and not ws_state['amax']:
                    ws[-2:].copy_(seed_ws[:2])
                    ws_state['amax'] = True
                if not (plus or scalable):
                    table = torch.from_numpy(fixed.copy()).to(sigs.device) if fixed is not None else self._random_init(st, V, rng)
                run = self._lloyd(st, table, max_iter, ws, ws_state)
                if best is None or run[2] < best[2]:
                    best = run
        table, lens, inertia, history = best
        self.fit_method, self.n_sig, self.cls_th = method, st.R, kw[D_CLS_TH[method]]
        self.n_iter_, self.inertia_, self.changed_ = len(history), inertia, history
        self.n_noise = self.labels_ = None
        self.centers, self.lens = table.cpu().numpy(), lens.cpu().numpy()
        return self
