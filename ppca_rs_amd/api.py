"""Python mirror of the reference's class surface for the EM hot path.

Same names, argument meaning and error behaviour as the PyO3 module
`ppca_rs.ppca_rs` (reference: src/python_bindings.rs:15-26) and the trainers of
python/ppca_rs/__init__.py, built over the C-ABI of include/ppca_hip.h.  All heavy
calls run on the GPU through libppca_hip.so; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import io
import math
from dataclasses import dataclass
from typing import Iterator, List, Literal, Optional, Sequence

import numpy as np

from . import _lib
from . import wire as _wire
from ._lib import check, f64, lib, ptr


def _ctx(ctx=None) -> _lib.Context:
    return ctx if ctx is not None else _lib.default_context()


# --------------------------------------------------------------------------- Dataset
class Dataset:
    """A device-resident dataset (reference: `Dataset`, src/python_bindings.rs:28-134).

    `Dataset(ndarray, weights=None)`: float64 (N, d); non-finite entries are masked
    (dataset.rs:19-22); weights default to 1 (dataset.rs:153-158).
    """

    def __init__(self, ndarray, weights=None, *, ctx=None, _handle=None):
        self._ctx = _ctx(ctx)
        if _handle is not None:
            self._h = _handle
            return
        arr = np.asarray(ndarray)
        if arr.dtype != np.float64:
            raise TypeError("Dataset expects a float64 array (reference: PyReadonlyArray2<f64>)")
        if arr.ndim != 2:
            raise TypeError("Dataset expects a 2-D array (n_samples, n_features)")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights), dtype=np.float64).ravel()
            if w.shape[0] != arr.shape[0]:
                raise ValueError("weights and data differ in length")  # assert_eq! dataset.rs:162
        if arr.shape[1] < 1:
            raise ValueError("Dataset needs at least one feature")
        h = C.c_void_p()
        es = arr.itemsize
        check(lib().ppca_dataset_from_host(self._ctx.handle, C.c_void_p(arr.ctypes.data), arr.shape[0], arr.shape[1],
                                           arr.strides[0] // es, arr.strides[1] // es, ptr(w), C.byref(h)))
        self._h = h

    @classmethod
    def _wrap(cls, handle, ctx) -> "Dataset":
        return cls(None, ctx=ctx, _handle=handle)

    @classmethod
    def from_device(cls, x_ptr: int, n: int, d: int, weights_ptr: int | None = None, *, ctx=None, keepalive=None):
        """Borrow device memory (e.g. a torch tensor's data_ptr()); `keepalive` is held."""
        c = _ctx(ctx)
        h = C.c_void_p()
        check(lib().ppca_dataset_from_device(c.handle, C.c_void_p(x_ptr), n, d,
                                             C.c_void_p(weights_ptr) if weights_ptr else None, C.byref(h)))
        ds = cls._wrap(h, c)
        ds._keepalive = keepalive
        return ds

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().ppca_dataset_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(lib().ppca_dataset_len(self._h))

    def output_size(self) -> Optional[int]:
        """dataset.rs:189-191 -- None for an empty dataset."""
        return int(lib().ppca_dataset_output_size(self._h)) if len(self) > 0 else None

    @property
    def _d(self) -> int:
        return int(lib().ppca_dataset_output_size(self._h))

    def numpy(self) -> np.ndarray:
        """(N, d) float64 with NaN at masked positions (src/python_bindings.rs:81-92)."""
        out = np.empty((len(self), self._d), dtype=np.float64)
        check(lib().ppca_dataset_to_host(self._h, ptr(out)))
        return out

    def weights(self) -> np.ndarray:
        out = np.empty(len(self), dtype=np.float64)
        check(lib().ppca_dataset_weights_to_host(self._h, ptr(out)))
        return out

    def with_weights(self, weights) -> "Dataset":
        """Same rows, new weights, no copy of the rows (dataset.rs:171-176)."""
        w = np.ascontiguousarray(np.asarray(weights), dtype=np.float64).ravel()
        if w.shape[0] != len(self):
            raise ValueError("weights and data differ in length")
        h = C.c_void_p()
        check(lib().ppca_dataset_with_weights(self._h, ptr(w), None, C.byref(h)))
        return Dataset._wrap(h, self._ctx)

    def empty_dimensions(self) -> List[int]:
        """Dimensions masked in every sample (dataset.rs:194-222)."""
        if len(self) == 0:
            return []
        flags = (C.c_int32 * self._d)()
        check(lib().ppca_dataset_empty_dimensions(self._h, flags))
        return [j for j in range(self._d) if flags[j]]

    def _scale_columns(self, a, b=None, l=None, *, out: bool = True, col_sums: bool = False, row_sums: bool = False):
        """ppca_dataset_scale_columns: (x * a as a new Dataset or None, (tot, sum, sq) of x * a - b or None, row sums of l over
        the observed entries or None) from one streaming pass."""
        d = self._d
        a, b, l = f64(a, (d,)), (f64(b, (d,)) if b is not None else None), (f64(l, (d,)) if l is not None else None)
        h = C.c_void_p()
        sums = np.empty((3, d)) if col_sums else None
        rows = np.empty(len(self)) if row_sums else None
        check(lib().ppca_dataset_scale_columns(self._ctx.handle, self._h, ptr(a), ptr(b), ptr(l), C.byref(h) if out else None,
                                               ptr(sums), ptr(rows)))
        return (Dataset._wrap(h, self._ctx) if out else None), sums, rows

    def holdout(self, fraction: float, seed: Optional[int] = None, *, row_offset: int = 0):
        """(train, held): the entry-wise hold-out split of cross-validation, in one streaming pass on the GPU.  Every observed entry
        is held with probability `fraction`, decided by a counter-based generator keyed by (seed, row_offset + row, column): a held
        entry is NaN in `train` and keeps its bits in `held`, a kept one the other way round, a masked one is NaN in both.  Both
        carry the input weights.  A slice starting at row s split with row_offset=s reproduces those rows of the whole.
        seed=None draws a fresh seed.  train.holdout_counts = held.holdout_counts = (entries kept, entries held)."""
        if not 0.0 <= float(fraction) <= 1.0:  # (NaN fails both comparisons)
            raise ValueError("fraction must lie in [0, 1]")
        return self._split(lib().ppca_dataset_holdout, (float(fraction),), seed, row_offset)

    def _split(self, entry, what, seed: Optional[int], row_offset: int):
        """The call of ppca_dataset_holdout / ppca_dataset_holdout_range (`what`: the fraction, or lo and hi) and its two datasets."""
        if row_offset < 0:
            raise ValueError("row_offset must be >= 0")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        th, hh = C.c_void_p(), C.c_void_p()
        counts = np.zeros(2)
        check(entry(self._ctx.handle, self._h, *what, int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), C.byref(th), C.byref(hh), ptr(counts)))
        train, held = Dataset._wrap(th, self._ctx), Dataset._wrap(hh, self._ctx)
        train.holdout_counts = held.holdout_counts = (int(counts[0]), int(counts[1]))
        return train, held

    def holdout_range(self, lo: float, hi: float, seed: Optional[int] = None, *, row_offset: int = 0):
        """`holdout` with the held entries those whose uniform u lies in [lo, hi) -- the same u, so holdout(f) is holdout_range(0, f)
        bit for bit, and ranges that share their edges are disjoint folds (`kfold`).  Requires 0 <= lo <= hi <= 1."""
        if not 0.0 <= float(lo) <= float(hi) <= 1.0:  # (NaN fails the comparisons)
            raise ValueError("the range must satisfy 0 <= lo <= hi <= 1")
        return self._split(lib().ppca_dataset_holdout_range, (float(lo), float(hi)), seed, row_offset)

    @staticmethod
    def fold_edges(n_folds: int):
        """The n_folds + 1 edges f / n_folds of `kfold`, the last one exactly 1.0."""
        n_folds = int(n_folds)
        if n_folds < 2:
            raise ValueError("n_folds must be >= 2")
        return [f / n_folds for f in range(n_folds)] + [1.0]

    def kfold(self, n_folds: int, seed: Optional[int] = None, *, row_offset: int = 0):
        """The n_folds (train, held) pairs of entry-wise K-fold cross-validation: fold f holds the observed entries whose uniform lies
        in [f / n_folds, (f + 1) / n_folds).  Neighbouring folds share an edge value and the last edge is exactly 1, so every observed
        entry is held in exactly one fold.  One streaming pass per fold; seed=None draws one fresh seed for all of them."""
        edges = Dataset.fold_edges(n_folds)
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        return [self.holdout_range(lo, hi, seed, row_offset=row_offset) for lo, hi in zip(edges, edges[1:])]

    def _fill_masked(self, fill: "Dataset", a) -> "Dataset":
        """ppca_dataset_fill_masked: this dataset's observed entries as they are, fill * a elsewhere."""
        h = C.c_void_p()
        check(lib().ppca_dataset_fill_masked(self._ctx.handle, self._h, fill._h, ptr(f64(a, (self._d,))), C.byref(h)))
        return Dataset._wrap(h, self._ctx)

    def _column_moments_multi(self, e, a=None, b=None) -> np.ndarray:
        """ppca_dataset_column_moments_multi: for K row-weight vectors e (K, N) used INSTEAD of the dataset's weights, a per-column
        factor a (d, default 1) and per-component offsets b (K, d, default 0), the (K, 3, d) sums tot / sum / sq of e m,
        e m (x a - b_c), e m (x a - b_c)^2 from one streaming pass over the dataset."""
        d, n = self._d, len(self)
        e = f64(e)
        if e.ndim != 2 or e.shape[1] != n or e.shape[0] < 1:
            raise ValueError(f"e must have shape (K, {n})")
        nc = e.shape[0]
        a = f64(a, (d,)) if a is not None else None
        b = f64(b, (nc, d)) if b is not None else None
        sums = np.empty((nc, 3, d))
        check(lib().ppca_dataset_column_moments_multi(self._ctx.handle, self._h, ptr(e), None, nc, ptr(a), ptr(b), ptr(sums)))
        return sums

    def column_stats(self):
        """(totals, means, variances) of every column over its observed entries, weighted: totals_j = sum_i w_i m_ij, the
        weighted mean, and the weighted mean of the squared deviations from it (0 for a column with no observed entry).  Two
        sums-only sweeps on the GPU (the second centred on the means of the first, so that the variance does not cancel)."""
        d = self._d
        one = np.ones(d)
        _, s1, _ = self._scale_columns(one, out=False, col_sums=True)
        tot = s1[0]
        safe = np.where(tot > 0.0, tot, 1.0)
        mean = np.where(tot > 0.0, s1[1] / safe, 0.0)
        _, s2, _ = self._scale_columns(one, mean, out=False, col_sums=True)
        var = np.where(tot > 0.0, s2[2] / safe - (s2[1] / safe) ** 2, 0.0)
        return tot, mean, np.maximum(var, 0.0)

    def pairwise_moments(self, center="mean", cross: bool = False) -> "PairwiseMoments":
        """The second moments between every two columns over the entries that are there, as one dense fp64 MFMA pass on the GPU
        (ppca_dataset_pairwise_moments): with x~ = x - center on observed entries, sums = sum_i w_i x~_ij x~_il over the rows where
        both are observed, counts = sum_i w_i m_ij m_il and, with cross=True (twice the work), cross = sum_i w_i x~_ij m_il.

        center="mean": the weighted column means over observed entries (0 for an empty column; one sums sweep); None: zeros; or an
        array of length d.  Nothing of the dataset comes to the host but the d x d results."""
        d = self._d
        if center is None:
            c = np.zeros(d)
        elif isinstance(center, str):
            if center != "mean":
                raise ValueError(f"center must be 'mean', None or an array of length {d}")
            _, s1, _ = self._scale_columns(np.ones(d), out=False, col_sums=True)
            c = np.where(s1[0] > 0.0, s1[1] / np.where(s1[0] > 0.0, s1[0], 1.0), 0.0)
        else:
            c = f64(center).reshape(-1)
            if c.shape[0] != d:
                raise ValueError(f"center must have length {d}")
        if not np.all(np.isfinite(c)):
            raise ValueError("every entry of center must be finite")
        sums, counts = np.empty((d, d)), np.empty((d, d))
        cr = np.empty((d, d)) if cross else None
        check(lib().ppca_dataset_pairwise_moments(self._ctx.handle, self._h, ptr(c), ptr(sums), ptr(counts), ptr(cr)))
        return PairwiseMoments(c, sums, counts, cr)

    def _kmeans_scale(self, scale) -> Optional[np.ndarray]:
        """The column scale of the k-means calls: None, "std" or an array of length d, checked."""
        d = self._d
        if scale is None:
            return None
        if isinstance(scale, str):
            if scale != "std":
                raise ValueError(f"scale must be None, 'std' or an array of length {d}")
            var = self.column_stats()[2]
            return np.where(var > 0.0, 1.0 / np.sqrt(np.where(var > 0.0, var, 1.0)), 1.0)
        a = f64(scale).reshape(-1)
        if a.shape[0] != d:
            raise ValueError(f"scale must have length {d}")
        if not np.all(np.isfinite(a)):
            raise ValueError("every entry of scale must be finite")
        return a

    def _kmeans_centers(self, centers) -> np.ndarray:
        d = self._d
        c = f64(centers)
        if c.ndim != 2 or c.shape[1] != d:
            raise ValueError(f"centers must have shape (K, {d})")
        if not 1 <= c.shape[0] <= 16:
            raise ValueError("the number of clusters must lie in 1 .. 16")
        if not np.all(np.isfinite(c)):
            raise ValueError("every entry of centers must be finite")
        return c

    def _kmeans_call(self, c: np.ndarray, a: Optional[np.ndarray], labels: bool, distances: bool, sums: bool) -> "KMeansStep":
        n, d, nc = len(self), self._d, c.shape[0]
        lab = np.zeros(n, dtype=np.int32) if labels else None
        dist = np.zeros(n) if distances else None
        out = np.zeros((nc, 2, d)) if sums else None
        inertia, reads = C.c_double(0.0), C.c_int32(0)
        check(lib().ppca_dataset_kmeans_step(self._ctx.handle, self._h, ptr(c), ptr(a), nc, ptr(lab), ptr(dist), ptr(out),
                                             C.byref(inertia), C.byref(reads)))
        return KMeansStep(c, out[:, 0] if sums else None, out[:, 1] if sums else None, inertia.value, labels=lab, distances=dist,
                          reads=int(reads.value))

    def kmeans_step(self, centers, scale=None, *, labels: bool = True, distances: bool = False) -> "KMeansStep":
        """One Lloyd iteration of masked k-means on the GPU (ppca_dataset_kmeans_step): every row goes to the centre nearest to it over
        the row's observed entries, dist_ic = sum_j m_ij (scale_j (x_ij - centers_cj))^2 (the lowest index on an exact tie; label 0 for a
        row with no observed entry), and every cluster's weighted column sums over the observed entries of its rows come from the same
        read of the dataset (d <= 512 and K <= 8; otherwise an assignment sweep and an update sweep per 8 centres: `reads`).

        centers: (K, d), K in 1 .. 16, finite; scale: None or an array of length d, finite.  labels / distances: fetch the rows' labels
        (int32) and distances to the host.  `KMeansStep.centers()` gives the updated centres.  A dataset without rows gives zeros (the
        steps of row blocks add up: `KMeansStep.__add__`)."""
        if isinstance(scale, str):
            raise TypeError("scale must be None or an array here; Dataset.kmeans resolves 'std'")
        return self._kmeans_call(self._kmeans_centers(centers), self._kmeans_scale(scale), bool(labels), bool(distances), True)

    def _kmeans_seed(self, n_clusters: int, u, a: Optional[np.ndarray]):
        """ppca_dataset_kmeans_seed: (centres (K, d), rows (K)) of k-means++ from the K numbers u in [0, 1)."""
        d = self._d
        u = f64(u, (n_clusters,))
        centers, rows = np.empty((n_clusters, d)), np.empty(n_clusters, dtype=np.int64)
        check(lib().ppca_dataset_kmeans_seed(self._ctx.handle, self._h, ptr(a), n_clusters, ptr(u), ptr(centers), ptr(rows)))
        return centers, rows

    def kmeans(self, n_clusters: int, *, n_iters: int = 20, seed: Optional[int] = None, scale=None, start=None) -> "KMeans":
        """Masked k-means on the GPU: k-means++ seeding on the device (`numpy.random.default_rng(seed).random(n_clusters)` are the
        numbers it picks with; `start`, (K, d) centres, replaces it), then at most `n_iters` Lloyd iterations of one `kmeans_step`
        each without fetching labels, stopping early when a step leaves every centre bit-identical, then one labelling call.

        scale: None; "std" (1 / the observed standard deviation of `column_stats()`, 1 for a column without variance: no column's
        unit dominates the distance); or an array of length d.  Every step decreases the weighted inertia (`history`: the inertia
        before each update); k-means has local optima, which a different seed may leave."""
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)):
            raise TypeError("n_clusters must be an integer")
        nc = int(n_clusters)
        if not 1 <= nc <= 16:
            raise ValueError("n_clusters must lie in 1 .. 16")
        if int(n_iters) < 0:
            raise ValueError("n_iters must be >= 0")
        if start is not None:
            centers = self._kmeans_centers(start).copy()
            if centers.shape[0] != nc:
                raise ValueError(f"start must have shape ({nc}, {self._d})")
        if len(self) == 0:
            raise ValueError("dataset is empty")
        a = self._kmeans_scale(scale)
        if start is None:
            centers, _ = self._kmeans_seed(nc, np.random.default_rng(seed).random(nc), a)
        history, converged = [], False
        for _ in range(int(n_iters)):
            step = self._kmeans_call(centers, a, False, False, True)
            history.append(step.inertia)
            new = step.centers()
            if np.array_equal(new, centers):
                converged = True
                break
            centers = new
        last = self._kmeans_call(centers, a, True, False, False)
        cw = np.bincount(last.labels, weights=self.weights(), minlength=nc).astype(np.float64)
        return KMeans(centers, last.labels, last.inertia, np.array(history), cw, len(history), converged)

    def covariance(self, mode: str = "global", ddof: float = 0.0, center="mean") -> np.ndarray:
        """`pairwise_moments(center, cross=(mode == "pairwise")).covariance(mode, ddof)`."""
        return self.pairwise_moments(center, cross=(mode == "pairwise")).covariance(mode, ddof)

    def correlation(self, mode: str = "global", center="mean") -> np.ndarray:
        """`pairwise_moments(center, cross=(mode == "pairwise")).correlation(mode)`."""
        return self.pairwise_moments(center, cross=(mode == "pairwise")).correlation(mode)

    def chunks(self, chunks: int) -> "DatasetChunks":
        """Iterator over ceil(N / chunks)-row slices (src/python_bindings.rs:110-118)."""
        return DatasetChunks(self, chunks)

    def _slice(self, start: int, length: int) -> "Dataset":
        h = C.c_void_p()
        check(lib().ppca_dataset_slice(self._h, start, length, C.byref(h)))
        ds = Dataset._wrap(h, self._ctx)
        ds._parent = self
        return ds

    @staticmethod
    def concat(datasets: Sequence["Dataset"]) -> "Dataset":
        """src/python_bindings.rs:121-133"""
        datasets = list(datasets)
        if not datasets:
            raise ValueError("cannot concatenate an empty list of datasets")
        ctx = datasets[0]._ctx
        arr = (C.c_void_p * len(datasets))(*[d._h for d in datasets])
        h = C.c_void_p()
        check(lib().ppca_dataset_concat(ctx.handle, arr, len(datasets), C.byref(h)))
        return Dataset._wrap(h, ctx)

    # dump/load (src/python_bindings.rs:66-79).  Default container: npz (round trip verified here);
    # format="bincode" writes the reference's bincode layout as restated in wire.py (parity unpinned: no real
    # artefact to check against).  load() accepts both.
    def dump(self, format: str = "npz") -> bytes:
        if format == "bincode":
            return _wire.dump_dataset(self.numpy(), self.weights())
        buf = io.BytesIO()
        np.savez(buf, kind="ppca_rs_amd.Dataset", data=self.numpy(), weights=self.weights())
        return buf.getvalue()

    @staticmethod
    def load(data: bytes) -> "Dataset":
        try:
            if bytes(data[:2]) != b"PK":
                x, w = _wire.load_dataset(data)
                return Dataset(x, w)
            z = np.load(io.BytesIO(data), allow_pickle=False)
            return Dataset(z["data"], z["weights"])
        except Exception as err:  # reference: bincode error -> Exception(str)
            raise Exception(str(err))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        other = Dataset.load(state)
        self._ctx, self._h = other._ctx, other._h
        other._h = None

    def __repr__(self):
        return f"Dataset(n={len(self)}, output_size={self.output_size()})"


class DatasetChunks:
    """src/python_bindings.rs:136-166"""

    def __init__(self, dataset: Dataset, chunks: int):
        if chunks <= 0:
            raise ValueError("chunks must be positive")
        self.dataset = dataset
        self.length = len(dataset)
        self.stride = int(math.ceil(self.length / chunks))
        self.position = 0

    def __iter__(self) -> Iterator[Dataset]:
        return self

    def __next__(self) -> Dataset:
        if self.position < self.length:
            n = min(self.length, self.position + self.stride) - self.position
            out = self.dataset._slice(self.position, n)
            self.position += self.stride
            return out
        raise StopIteration


# --------------------------------------------------------------------------- row-compressed data
class SparseDataset:
    """A dataset in CSR form (an extension with no reference counterpart): of an N x n_columns matrix only the entries
    that exist are stored, everything else is masked.  For data of which a few percent exists (ratings, purchases, assays), where the
    dense N x d form of `Dataset` does not fit the device or is almost all NaN.

    `SparseDataset(indptr, indices, values, n_columns, weights=None)`: indptr (N + 1, monotone from 0 to nnz), indices (nnz, strictly
    increasing within a row, in [0, n_columns)), values (nnz, finite).  Anything else raises ValueError before the library is touched.
    block_rows / segment: the two tiling lengths of the passes (None: the library's defaults; tests put the seams at small sizes).
    The entries go to the device, with the inverted index the statistics pass reads, on first use.
    `SparseDataset.from_device(indptr_ptr, indices_ptr, values_ptr, n, n_columns)` borrows CSR arrays that already live on the device
    and validates them and builds the index there: such a dataset holds no host arrays (csr() and its like fetch them
    on first use), every method that takes a SparseDataset takes it with the same bits, and its hold-out splits run on the device.
    `holdout` / `holdout_range` / `kfold` split the entries (on the host, or with on_device=True on the device) exactly as Dataset's
    split the same matrix, and
    PPCAModel.heldout_score takes the two parts.  PPCAMix takes one too: llk / llks / infer_cluster / iterate* /
    predict and PPCAMixTrainer.  So does FAModel, one noise level per column: llk / llks / infer / iterate* / predict /
    heldout_score and FATrainer.  So does TPPCAModel, the robust model: llk / llks / row_weights / mahalanobis / infer /
    predict / iterate* and TPPCATrainer.train.  So does HPPCAModel, with a known precision per stored entry: llk / llks /
    infer / predict / iterate* and HPPCATrainer.train take (sparse, precisions); `with_values` lets the precisions
    travel as a SparseDataset of the same pattern."""

    def __init__(self, indptr, indices, values, n_columns: int, weights=None, *, ctx=None, block_rows: Optional[int] = None,
                 segment: Optional[int] = None):
        ip = np.asarray(indptr)
        ix = np.asarray(indices)
        v = np.asarray(values)
        if ip.ndim != 1 or ix.ndim != 1 or v.ndim != 1:
            raise ValueError("indptr, indices and values must be 1-D")
        if ip.size < 1 or (ip.size and not np.issubdtype(ip.dtype, np.integer)) or (ix.size and not np.issubdtype(ix.dtype, np.integer)):
            raise ValueError("indptr (at least one element) and indices must be integer arrays")
        d = int(n_columns)
        if d < 1 or d >= 2 ** 31:
            raise ValueError("n_columns must lie in [1, 2^31)")
        ip = np.ascontiguousarray(ip, dtype=np.int64)
        n = ip.size - 1
        if ip[0] != 0 or np.any(np.diff(ip) < 0):
            raise ValueError("indptr must start at 0 and be monotone")
        if ip[-1] != ix.size or ix.size != v.size:
            raise ValueError("indptr[-1], len(indices) and len(values) differ")
        if ix.size and (ix.min() < 0 or ix.max() >= d):
            raise ValueError(f"a column index lies outside [0, {d})")
        ix = np.ascontiguousarray(ix, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.float64)
        if ix.size > 1:
            inc = np.diff(ix) > 0
            inc[ip[1:-1][(ip[1:-1] > 0) & (ip[1:-1] < ix.size)] - 1] = True  # (the step from one row's last entry to the next row's first)
            if not inc.all():
                raise ValueError("column indices must be strictly increasing within a row (sorted, no duplicates)")
        if not np.isfinite(v).all():
            raise ValueError("values must be finite (an entry that is missing is simply not stored)")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights), dtype=np.float64).ravel()
            if w.shape[0] != n:
                raise ValueError("weights and data differ in length")
        for name, val in (("block_rows", block_rows), ("segment", segment)):
            if val is not None and int(val) < 1:
                raise ValueError(f"{name} must be positive")
        for a in (ip, ix, v):
            a.setflags(write=False)
        self._ip, self._ix, self._vals, self._d, self._wts = ip, ix, v, d, w
        self._on_device = False
        self._block_rows, self._segment = int(block_rows or 0), int(segment or 0)
        self._ctx_arg = ctx
        self._handle = None

    # -- construction ---------------------------------------------------------
    @classmethod
    def from_dense(cls, ndarray, weights=None, **kw) -> "SparseDataset":
        """The finite entries of an (N, d) array; non-finite ones are dropped (they are what `Dataset` masks)."""
        x = np.asarray(ndarray, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("from_dense expects a 2-D array")
        obs = np.isfinite(x)
        indptr = np.concatenate([[0], np.cumsum(obs.sum(axis=1))]).astype(np.int64)
        return cls(indptr, np.nonzero(obs)[1].astype(np.int32), x[obs], x.shape[1], weights, **kw)

    @classmethod
    def from_coo(cls, rows, cols, values, shape, weights=None, **kw) -> "SparseDataset":
        """From (row, column, value) triplets in any order; a position given twice raises ValueError."""
        r = np.asarray(rows).astype(np.int64).ravel()
        c = np.asarray(cols).astype(np.int64).ravel()
        v = np.asarray(values, dtype=np.float64).ravel()
        n, d = int(shape[0]), int(shape[1])
        if not (r.size == c.size == v.size):
            raise ValueError("rows, cols and values differ in length")
        if r.size and (r.min() < 0 or r.max() >= n):
            raise ValueError(f"a row index lies outside [0, {n})")
        order = np.lexsort((c, r))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
        return cls(indptr, c[order], v[order], d, weights, **kw)

    @classmethod
    def from_device(cls, indptr_ptr: int, indices_ptr: int, values_ptr: int, n: int, n_columns: int, weights_ptr: Optional[int] = None, *,
                    ctx=None, keepalive=None, block_rows: Optional[int] = None, segment: Optional[int] = None) -> "SparseDataset":
        """Borrow CSR arrays that live on the device (e.g. three torch tensors' data_ptr(): indptr int64 (n + 1), indices int32 and
        values float64 (nnz each), weights float64 (n) or None); `keepalive` is held, and handed on to every dataset made from this
        one.  The format is validated and the index built on the device: a violation raises PPCAError naming the lowest
        offending row.  The dataset holds a handle and no host arrays: csr(), to_dense(), with_values and the host-side split fetch
        them on first use; its hold-out splits run on the device."""
        n, d = int(n), int(n_columns)
        if not indptr_ptr:
            raise ValueError("indptr_ptr is null")
        if n < 0:
            raise ValueError("n must be >= 0")
        if d < 1 or d >= 2 ** 31:
            raise ValueError("n_columns must lie in [1, 2^31)")
        for name, val in (("block_rows", block_rows), ("segment", segment)):
            if val is not None and int(val) < 1:
                raise ValueError(f"{name} must be positive")
        c = _ctx(ctx)
        h = C.c_void_p()
        check(lib().ppca_from_device_sparse(n, d, c.handle, C.c_void_p(indptr_ptr), C.c_void_p(indices_ptr) if indices_ptr else None,
                                            C.c_void_p(values_ptr) if values_ptr else None, C.c_void_p(weights_ptr) if weights_ptr else None,
                                            int(block_rows or 0), int(segment or 0), C.byref(h)))
        return cls._device_born(h, c, d, int(block_rows or 0), int(segment or 0), weights=bool(weights_ptr), keepalive=keepalive)

    @classmethod
    def _device_born(cls, handle, ctx, d: int, block_rows: int, segment: int, *, weights, keepalive) -> "SparseDataset":
        """A dataset around a handle the library built on the device.  weights: False (all ones), True (on the device: fetched on
        first use) or the host copy."""
        out = cls.__new__(cls)
        out._ip = out._ix = out._vals = None
        out._wts = None if isinstance(weights, bool) else weights
        out._w_on_device = weights is True
        out._d, out._block_rows, out._segment = d, block_rows, segment
        out._ctx_arg, out._handle, out._on_device, out._keepalive = ctx, handle, True, keepalive
        return out

    def _fetch(self) -> None:
        """The pattern and the weights of a device-born dataset, to the host (once)."""
        if self._ip is None:
            n, nnz = int(lib().ppca_sparse_len(self._handle)), int(lib().ppca_sparse_nnz(self._handle))
            ip, ix = np.empty(n + 1, dtype=np.int64), np.empty(nnz, dtype=np.int32)
            check(lib().ppca_sparse_to_host(self._handle, ptr(ip), ptr(ix), None, None))
            ip.setflags(write=False)
            ix.setflags(write=False)
            self._ip, self._ix = ip, ix
        if getattr(self, "_w_on_device", False):
            w = np.empty(len(self))
            check(lib().ppca_sparse_to_host(self._handle, None, None, None, ptr(w)))
            self._wts, self._w_on_device = w, False

    # the host arrays: a device-born dataset downloads them on first use
    @property
    def _indptr(self) -> np.ndarray:
        self._fetch()
        return self._ip

    @_indptr.setter
    def _indptr(self, a):
        self._ip = a

    @property
    def _indices(self) -> np.ndarray:
        self._fetch()
        return self._ix

    @_indices.setter
    def _indices(self, a):
        self._ix = a

    @property
    def _w(self) -> Optional[np.ndarray]:
        if getattr(self, "_w_on_device", False):
            self._fetch()
        return self._wts

    @_w.setter
    def _w(self, w):
        self._wts, self._w_on_device = w, False

    # -- the device handle ----------------------------------------------------
    @property
    def _ctx(self) -> _lib.Context:
        if self._ctx_arg is None:
            self._ctx_arg = _ctx(None)
        return self._ctx_arg

    @property
    def _h(self):
        # every pass written for the dense layout reaches its dataset through _h
        raise TypeError("this operation is not available on a SparseDataset (DESIGN.md section 7); PPCAModel.llk / llks / infer / iterate* / "
                        "predict / recommend / heldout_score and PPCATrainer are, and PPCAMix.llk / llks / infer_cluster / iterate* / "
                        "predict / recommend and PPCAMixTrainer, and FAModel.llk / llks / infer / iterate* / predict / heldout_score and "
                        "FATrainer, and TPPCAModel.llk / llks / row_weights / mahalanobis / infer / predict / iterate* and TPPCATrainer.train, "
                        "and HPPCAModel.llk / llks / infer / predict / iterate* and HPPCATrainer.train with (sparse, precisions)")

    @property
    def _values(self) -> np.ndarray:
        """The values on the host.  A values view (`_scale_columns`) is made on the device and fetches them on first use only."""
        if self._vals is None:
            v = np.empty(self.nnz)
            check(lib().ppca_sparse_to_host(self._handle, None, None, ptr(v), None))
            v.setflags(write=False)
            self._vals = v
        return self._vals

    @_values.setter
    def _values(self, v):
        self._vals = v

    @property
    def _sh(self):
        if self._handle is None:
            h = C.c_void_p()
            check(lib().ppca_sparse_from_host(self._ctx.handle, len(self), self._d, ptr(self._indptr), ptr(self._indices), ptr(self._values),
                                              ptr(self._w), self._block_rows, self._segment, C.byref(h)))
            self._handle = h
        return self._handle

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                lib().ppca_sparse_free(self._handle)
                self._handle = None
        except Exception:
            pass

    # -- accessors ------------------------------------------------------------
    def __len__(self) -> int:
        return int(self._ip.size - 1) if self._ip is not None else int(lib().ppca_sparse_len(self._handle))

    def output_size(self) -> Optional[int]:
        return self._d if len(self) > 0 else None

    @property
    def nnz(self) -> int:
        return int(self._ix.size) if self._ix is not None else int(lib().ppca_sparse_nnz(self._handle))

    def csr(self):
        """(indptr int64, indices int32, values float64): copies."""
        return self._indptr.copy(), self._indices.copy(), self._values.copy()

    def weights(self) -> np.ndarray:
        return np.ones(len(self)) if self._w is None else self._w.copy()

    def with_weights(self, weights) -> "SparseDataset":
        """Same entries (and, once built, the same device copy and index), new weights."""
        w = np.ascontiguousarray(np.asarray(weights), dtype=np.float64).ravel()
        if w.shape[0] != len(self):
            raise ValueError("weights and data differ in length")
        out = SparseDataset.__new__(SparseDataset)
        out.__dict__.update(self.__dict__)
        out._w, out._handle = w, None
        if self._handle is not None:
            h = C.c_void_p()
            check(lib().ppca_sparse_with_weights(self._handle, ptr(w), C.byref(h)))
            out._handle = h
        return out

    def with_values(self, values) -> "SparseDataset":
        """Same pattern, weights, tiling and ctx, new values (nnz, finite, aligned with csr()[2]).  Host work: no device is touched and
        the new dataset uploads on first use.  This is how per-entry quantities travel with the data -- the precisions of HPPCAModel:
        `sp.with_values(p).holdout(f, seed)` splits p exactly as `sp.holdout(f, seed)` splits sp, because the split is keyed by
        (seed, row, column)."""
        v = np.ascontiguousarray(np.asarray(values), dtype=np.float64)
        if v.ndim != 1 or v.shape[0] != self.nnz:
            raise ValueError(f"values must be 1-D of length nnz = {self.nnz}; got shape {v.shape}")
        if not np.isfinite(v).all():
            raise ValueError("values must be finite (an entry that is missing is simply not stored)")
        v = v.copy()
        v.setflags(write=False)
        self._fetch()  # (the new dataset has no handle to fetch its pattern through)
        out = SparseDataset.__new__(SparseDataset)
        out.__dict__.update(self.__dict__)
        out.__dict__.pop("holdout_counts", None)
        out._vals, out._handle = v, None
        return out

    def empty_dimensions(self) -> List[int]:
        """Columns without an entry."""
        if len(self) == 0:
            return []
        return np.flatnonzero(np.bincount(self._indices, minlength=self._d) == 0).tolist()

    def _scale_columns(self, a, b=None, l=None, *, out: bool = True, col_sums: bool = False, row_sums: bool = False):
        """ppca_scale_columns_sparse, with Dataset._scale_columns's return triple: (the entries times a[column] as a SparseDataset or
        None, (tot, sum, sq) of x * a - b per column or None, the row sums of l over the row's entries or None), from one pass on the
        device.  The returned dataset is a values view: it shares this one's pattern, inverted index and weights on
        the device and only its values are new; they come to the host if csr() / to_dense() asks for them, not before."""
        d = self._d
        a, b, l = f64(a, (d,)), (f64(b, (d,)) if b is not None else None), (f64(l, (d,)) if l is not None else None)
        for name, v in (("a", a), ("b", b), ("l", l)):
            if v is not None and not np.isfinite(v).all():
                raise ValueError(f"every entry of {name} must be finite")
        if not (out or col_sums or row_sums):
            raise ValueError("no output requested")
        h = C.c_void_p()
        sums = np.empty((3, d)) if col_sums else None
        rows = np.empty(len(self)) if row_sums else None
        check(lib().ppca_scale_columns_sparse(self._ctx.handle, self._sh, ptr(a), ptr(b), ptr(l), C.byref(h) if out else None,
                                              ptr(sums), ptr(rows)))
        view = None
        if out:
            view = SparseDataset.__new__(SparseDataset)
            view.__dict__.update(self.__dict__)
            view.__dict__.pop("holdout_counts", None)
            view._vals, view._handle = None, h
        return view, sums, rows

    def column_stats(self):
        """(totals, means, variances) of every column over its entries, weighted: Dataset.column_stats on row-compressed data.  Two
        sums-only passes on the device, the second centred on the means of the first."""
        d = self._d
        one = np.ones(d)
        _, s1, _ = self._scale_columns(one, out=False, col_sums=True)
        tot = s1[0]
        safe = np.where(tot > 0.0, tot, 1.0)
        mean = np.where(tot > 0.0, s1[1] / safe, 0.0)
        _, s2, _ = self._scale_columns(one, mean, out=False, col_sums=True)
        var = np.where(tot > 0.0, s2[2] / safe - (s2[1] / safe) ** 2, 0.0)
        return tot, mean, np.maximum(var, 0.0)

    # -- hold-out splits ---------------------------------------
    def _select(self, keep: np.ndarray) -> "SparseDataset":
        """The entries flagged in `keep` (bool, nnz) as a SparseDataset with this one's weights, n_columns, ctx and tiling; values keep
        their bits.  No device work: the part uploads on first use."""
        self._fetch()  # (a device-born dataset: its pattern and weights, before the part is cut loose from the handle)
        out = SparseDataset.__new__(SparseDataset)
        out.__dict__.update(self.__dict__)
        out._handle = None
        out._indptr = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])[self._indptr]
        out._indices, out._values = self._indices[keep], self._values[keep]
        for a in (out._indptr, out._indices, out._values):
            a.setflags(write=False)
        return out

    def _split(self, lo: float, hi: float, seed: Optional[int], row_offset: int, on_device: Optional[bool] = None):
        """The call of ppca_heldout_split_csr_host (host code) and the two parts; on the device (on_device, or None on a device-born
        dataset or a part of one) the call of ppca_heldout_split_sparse, whose parts are device-born."""
        if row_offset < 0:
            raise ValueError("row_offset must be >= 0")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        if getattr(self, "_on_device", False) if on_device is None else on_device:
            th, hh, counts = C.c_void_p(), C.c_void_p(), np.zeros(2, dtype=np.int64)
            check(lib().ppca_heldout_split_sparse(float(lo), float(hi), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), self._ctx.handle,
                                                  self._sh, C.byref(th), C.byref(hh), ptr(counts)))
            weights = True if getattr(self, "_w_on_device", False) else (self._wts if self._wts is not None else False)
            parts = [SparseDataset._device_born(h, self._ctx, self._d, self._block_rows, self._segment, weights=weights,
                                                keepalive=getattr(self, "_keepalive", None)) for h in (th, hh)]
            parts[0].holdout_counts = parts[1].holdout_counts = (int(counts[0]), int(counts[1]))
            return parts[0], parts[1]
        flags, counts = np.zeros(self.nnz, dtype=np.uint8), np.zeros(2, dtype=np.int64)
        check(lib().ppca_heldout_split_csr_host(len(self), ptr(self._indptr), ptr(self._indices), float(lo), float(hi),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), ptr(flags), ptr(counts)))
        held = flags.view(np.bool_)
        train, heldp = self._select(~held), self._select(held)
        train.holdout_counts = heldp.holdout_counts = (int(counts[0]), int(counts[1]))
        return train, heldp

    def holdout(self, fraction: float, seed: Optional[int] = None, *, row_offset: int = 0, on_device: Optional[bool] = None):
        """(train, held): Dataset.holdout on row-compressed data.  Every entry is held with probability `fraction`, decided by the
        same word of the counter-based generator, keyed by (seed, row_offset + row, column): SparseDataset.from_dense(x).holdout(f, s)
        holds exactly the entries Dataset(x).holdout(f, s) holds.  Both parts are SparseDatasets with this one's weights, n_columns
        and tiling; the split is host work and touches no device.  seed=None draws a fresh seed.
        train.holdout_counts = held.holdout_counts = (entries kept, entries held).
        on_device: None = on the device for a device-born dataset (`from_device`) or a part of one, on the host otherwise; True forces
        the device split (a host-born dataset uploads first), whose parts are device-born: the same entries, the same value bits."""
        if not 0.0 <= float(fraction) <= 1.0:  # (NaN fails both comparisons)
            raise ValueError("fraction must lie in [0, 1]")
        return self._split(0.0, fraction, seed, row_offset, on_device)

    def holdout_range(self, lo: float, hi: float, seed: Optional[int] = None, *, row_offset: int = 0, on_device: Optional[bool] = None):
        """`holdout` with the held entries those whose uniform u lies in [lo, hi) (Dataset.holdout_range).  Requires 0 <= lo <= hi <= 1."""
        if not 0.0 <= float(lo) <= float(hi) <= 1.0:  # (NaN fails the comparisons)
            raise ValueError("the range must satisfy 0 <= lo <= hi <= 1")
        return self._split(lo, hi, seed, row_offset, on_device)

    fold_edges = staticmethod(Dataset.fold_edges)

    def kfold(self, n_folds: int, seed: Optional[int] = None, *, row_offset: int = 0, on_device: Optional[bool] = None):
        """The n_folds (train, held) pairs of entry-wise K-fold cross-validation (Dataset.kfold): every entry is held in exactly one
        fold.  seed=None draws one fresh seed for all of them.  on_device: as `holdout`."""
        edges = Dataset.fold_edges(n_folds)
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        return [self.holdout_range(lo, hi, seed, row_offset=row_offset, on_device=on_device) for lo, hi in zip(edges, edges[1:])]

    def index_build_seconds(self) -> float:
        """Time the constructor of the device copy spent on the inverted index, the row lists and the work items: host time for a
        host-born dataset, the wall time of the device build (its waits included) for a device-born one."""
        return float(lib().ppca_sparse_build_seconds(self._sh))

    def _dense(self) -> np.ndarray:
        x = np.full((len(self), self._d), np.nan)
        x[np.repeat(np.arange(len(self)), np.diff(self._indptr)), self._indices] = self._values
        return x

    def to_dense(self) -> Dataset:
        """The same data as a `Dataset` (NaN where there is no entry), with the same weights."""
        return Dataset(self._dense(), self._w, ctx=self._ctx)

    def __repr__(self):
        return f"SparseDataset(n={len(self)}, output_size={self.output_size()}, nnz={self.nnz})"


def _dense_only(*datasets):
    """Raises SparseDataset._h's TypeError before anything touches the device."""
    for ds in datasets:
        if isinstance(ds, SparseDataset):
            ds._h


def _query_pattern(sparse: SparseDataset, query):
    """(indptr int64, indices int32) of a predict query: a SparseDataset or an (indptr, indices) pair with the rows of `sparse`."""
    if isinstance(query, SparseDataset):
        ip, ix = query._indptr, query._indices
        if query._d != sparse._d:
            raise ValueError("query and data differ in the number of columns")
    else:
        ip = np.ascontiguousarray(np.asarray(query[0]), dtype=np.int64)
        ix = np.ascontiguousarray(np.asarray(query[1]), dtype=np.int32)
    if ip.ndim != 1 or ip.size != len(sparse) + 1:
        raise ValueError("query and data differ in the number of rows")
    if ip[0] != 0 or np.any(np.diff(ip) < 0) or ip[-1] != ix.size:
        raise ValueError("query indptr must be monotone from 0 to len(indices)")
    if ix.size and (ix.min() < 0 or ix.max() >= sparse._d):
        raise ValueError(f"a query column lies outside [0, {sparse._d})")
    return ip, ix


# --------------------------------------------------------------------------- pairwise second moments
class PairwiseMoments:
    """What `Dataset.pairwise_moments` returns, host arrays: `center` (d) and the d x d matrices `sums`, `counts` and (optional)
    `cross` of include/ppca_hip.h, ppca_dataset_pairwise_moments.  Constructible from host arrays; the sums are additive over row
    blocks (`a + b` for two results with the same centre: chunks, shards)."""

    def __init__(self, center, sums, counts, cross=None):
        c = np.array(center, dtype=np.float64).reshape(-1)
        d = c.shape[0]
        self._center = c
        self._sums = np.array(sums, dtype=np.float64).reshape(d, d)
        self._counts = np.array(counts, dtype=np.float64).reshape(d, d)
        self._cross = np.array(cross, dtype=np.float64).reshape(d, d) if cross is not None else None
        for a in (self._center, self._sums, self._counts, self._cross):
            if a is not None:
                a.setflags(write=False)

    @property
    def center(self) -> np.ndarray:
        return self._center.copy()

    @property
    def sums(self) -> np.ndarray:
        return self._sums.copy()

    @property
    def counts(self) -> np.ndarray:
        return self._counts.copy()

    @property
    def cross(self) -> Optional[np.ndarray]:
        return self._cross.copy() if self._cross is not None else None

    def __add__(self, other: "PairwiseMoments") -> "PairwiseMoments":
        if not isinstance(other, PairwiseMoments):
            return NotImplemented
        if self._center.shape != other._center.shape or not np.array_equal(self._center, other._center):
            raise ValueError("the two results are centred differently: their sums do not add")
        both = self._cross is not None and other._cross is not None
        return PairwiseMoments(self._center, self._sums + other._sums, self._counts + other._counts,
                               self._cross + other._cross if both else None)

    def covariance(self, mode: str = "global", ddof: float = 0.0) -> np.ndarray:
        """"global": sums / (counts - ddof), the second moment around the common centre over the rows where both columns are
        observed.  "pairwise" (needs `cross`): (sums - cross o cross^T / counts) / (counts - ddof), each pair centred on its own
        means over the co-observed rows -- with unit weights and ddof=1 what pandas.DataFrame.cov() computes.  NaN where
        counts <= ddof."""
        with np.errstate(divide="ignore", invalid="ignore"):
            if mode == "global":
                num = self._sums
            elif mode == "pairwise":
                if self._cross is None:
                    raise ValueError("mode='pairwise' needs cross: pairwise_moments(cross=True)")
                num = self._sums - self._cross * self._cross.T / self._counts
            else:
                raise ValueError("mode must be 'global' or 'pairwise'")
            return np.where(self._counts > ddof, num / (self._counts - ddof), np.nan)

    def correlation(self, mode: str = "global") -> np.ndarray:
        """cov_jl / sqrt(cov_jj cov_ll) of `covariance(mode)`.  NOT pandas' pairwise `corr`, which rescales each pair by the
        variances over the pair's co-observed rows only (a fourth matrix); here every pair is rescaled by the two columns' own
        variances over all their observed rows."""
        cov = self.covariance(mode)
        with np.errstate(divide="ignore", invalid="ignore"):
            sd = np.sqrt(np.diag(cov))
            return cov / np.outer(sd, sd)


# --------------------------------------------------------------------------- masked k-means
class KMeansStep:
    """What `Dataset.kmeans_step` returns, host arrays: `labels` (int32 N, or None), `distances` (N, or None), `totals` and `sums`
    ((K, d): tot_cj = sum of w_i over the rows of cluster c that observe column j, sum_cj = the same sum of w_i (x_ij - centre_cj),
    unscaled and centred on the centre the step was taken from), `inertia` (sum_i w_i dist_i) and `reads` (sweeps over the dataset).
    `a + b` adds the totals, sums and inertia of two steps taken with the same centres (chunks, shards); labels are dropped."""

    def __init__(self, centers, totals, sums, inertia, *, labels=None, distances=None, reads: int = 0):
        self._centers = np.array(centers, dtype=np.float64)
        if self._centers.ndim != 2:
            raise ValueError("centers must have shape (K, d)")
        shape = self._centers.shape
        self.totals = np.array(totals, dtype=np.float64).reshape(shape) if totals is not None else None
        self.sums = np.array(sums, dtype=np.float64).reshape(shape) if sums is not None else None
        self.inertia = float(inertia)
        self.labels = labels
        self.distances = distances
        self.reads = int(reads)

    def centers(self) -> np.ndarray:
        """The updated centres: centre_cj + sum_cj / tot_cj where tot_cj > 0, the old centre_cj elsewhere (an empty cluster, or a
        column a cluster never observes, keeps its value)."""
        if self.totals is None:
            return self._centers.copy()
        ok = self.totals > 0.0
        return np.where(ok, self._centers + self.sums / np.where(ok, self.totals, 1.0), self._centers)

    def __add__(self, other: "KMeansStep") -> "KMeansStep":
        if not isinstance(other, KMeansStep):
            return NotImplemented
        if self._centers.shape != other._centers.shape or not np.array_equal(self._centers, other._centers):
            raise ValueError("the two steps were taken with different centres: their sums do not add")
        if self.totals is None or other.totals is None:
            raise ValueError("a step without sums does not add")
        return KMeansStep(self._centers, self.totals + other.totals, self.sums + other.sums, self.inertia + other.inertia,
                          reads=max(self.reads, other.reads))


@dataclass
class KMeans:
    """What `Dataset.kmeans` returns: `centers` (K, d), the final `labels` (int32 N) and `inertia`, `history` (the inertia before each
    update), `cluster_weights` (the sum of w over each cluster's rows), `n_iters_run` and `converged` (a step left every centre
    bit-identical)."""

    centers: np.ndarray
    labels: np.ndarray
    inertia: float
    history: np.ndarray
    cluster_weights: np.ndarray
    n_iters_run: int
    converged: bool


def _kmeans_cluster_moments(dataset: Dataset, km: KMeans):
    """([the pairwise moments of every cluster's rows, None for a cluster of weight 0], the whole dataset's where one is needed, the
    log-weights of the start): K moment passes over the dataset with the weights w * (labels == c) -- rows of weight 0 add exactly
    nothing there.  A cluster of weight 0 gets the weight of the lightest cluster that has some."""
    labels = np.asarray(km.labels)
    if labels.shape != (len(dataset),):
        raise ValueError("km.labels and the dataset differ in length")
    w = dataset.weights()
    cw = np.asarray(km.cluster_weights, dtype=np.float64)
    if not np.any(cw > 0.0):
        raise ValueError("no cluster has any weight")
    moms = [dataset.with_weights(w * (labels == c)).pairwise_moments() if cw[c] > 0.0 else None for c in range(cw.shape[0])]
    whole = dataset.pairwise_moments() if any(m is None for m in moms) else None
    cw = np.where(cw > 0.0, cw, cw[cw > 0.0].min())
    return moms, whole, np.log(cw / cw.sum())


def _spectral_start(sigma_mat: np.ndarray, live: np.ndarray, k: int):
    """The closed-form maximum-likelihood PPCA model of a covariance matrix (Tipping and Bishop 1999) on its live columns:
    (sigma, C) with C (d x k), zero rows on the other columns and zero columns beyond the live ones."""
    d = sigma_mat.shape[0]
    c = np.zeros((d, k))
    idx = np.flatnonzero(live)
    dl = idx.shape[0]
    if dl == 0:
        return 1.0, c
    sub = np.nan_to_num(sigma_mat[np.ix_(idx, idx)], nan=0.0, posinf=0.0, neginf=0.0)
    trace = float(np.trace(sub))
    if not trace > 0.0:
        return 1.0, c
    lam, u = np.linalg.eigh(0.5 * (sub + sub.T))
    lam, u = lam[::-1], u[:, ::-1]
    floor = 1e-8 * trace / dl
    s2 = max(float(np.mean(lam[k:])), floor) if k < dl else floor
    kk = min(k, dl)
    c[idx, :kk] = u[:, :kk] * np.sqrt(np.maximum(lam[:kk] - s2, 0.0))
    return math.sqrt(s2), c


# --------------------------------------------------------------------------- Prior
class Prior:
    """MAP priors (prior.rs:8-65; src/python_bindings.rs:168-201).  Builders return a new Prior."""

    def __init__(self):
        self.mean: Optional[np.ndarray] = None
        self.mean_covariance: Optional[np.ndarray] = None
        self.isotropic_noise_alpha: Optional[float] = None
        self.isotropic_noise_beta: Optional[float] = None
        self.transformation_precision: float = 0.0

    def _copy(self) -> "Prior":
        p = Prior()
        p.__dict__.update(self.__dict__)
        return p

    def with_mean_prior(self, mean, mean_covariance) -> "Prior":
        mean = f64(mean).ravel()  # the reference wants 2-D row/column; 1-D is accepted too
        cov = f64(mean_covariance)
        if cov.shape != (mean.shape[0], mean.shape[0]):
            raise ValueError("mean covariance must be (d, d)")  # assert_eq! prior.rs:33-34
        if not np.isfinite(np.linalg.cond(cov)) or np.linalg.matrix_rank(cov) < cov.shape[0]:
            raise ValueError("mean covariance should be invertible")  # prior.rs:40
        p = self._copy()
        p.mean, p.mean_covariance = mean, cov
        return p

    def with_isotropic_noise_prior(self, alpha: float, beta: float) -> "Prior":
        if not (alpha >= 0.0 and beta >= 0.0):
            raise ValueError("alpha and beta must be >= 0")  # prior.rs:50-51
        p = self._copy()
        p.isotropic_noise_alpha, p.isotropic_noise_beta = float(alpha), float(beta)
        return p

    def with_transformation_precision(self, precision: float) -> "Prior":
        if not precision >= 0.0:
            raise ValueError("precision must be >= 0")  # prior.rs:61
        p = self._copy()
        p.transformation_precision = float(precision)
        return p

    def _c(self):
        c = _lib.Prior()
        c.has_mean_prior = int(self.mean is not None)
        if self.mean is not None:
            c.mean = self.mean.ctypes.data_as(_lib.c_double_p)
            c.mean_covariance = self.mean_covariance.ctypes.data_as(_lib.c_double_p)
        c.has_isotropic_noise_prior = int(self.isotropic_noise_alpha is not None)
        c.isotropic_noise_alpha = self.isotropic_noise_alpha or 0.0
        c.isotropic_noise_beta = self.isotropic_noise_beta or 0.0
        c.transformation_precision = self.transformation_precision
        return c


def _prior_ref(prior: Optional[Prior]):
    if prior is None:
        return None, None
    c = prior._c()
    return C.byref(c), c


# --------------------------------------------------------------------------- PPCAModel
class _DevModel:
    def __init__(self, handle):
        self.h = handle

    def __del__(self):
        try:
            if self.h:
                lib().ppca_model_free(self.h)
                self.h = None
        except Exception:
            pass


def _recommend_args(sparse, n, kappa, candidates):
    """The argument checks PPCAModel.recommend and PPCAMix.recommend share, in their documented order -> (n, kappa, candidates int32 or
    None); nothing here touches the library or a device."""
    if not isinstance(sparse, SparseDataset):
        raise TypeError("recommend takes a SparseDataset (from a Dataset or an array: SparseDataset.from_dense)")
    n = int(n)
    if not 1 <= n <= 64:
        raise ValueError("n must lie in [1, 64]")
    kappa = float(kappa)
    if not math.isfinite(kappa):
        raise ValueError("kappa must be finite")
    cand = None
    if candidates is not None:
        cand = np.asarray(candidates)
        if cand.ndim != 1 or (cand.size and not np.issubdtype(cand.dtype, np.integer)):
            raise ValueError("candidates must be a 1-D integer array")
        if cand.size and (cand.min() < 0 or cand.max() >= sparse._d):
            raise ValueError(f"a candidate column lies outside [0, {sparse._d})")
        if np.any(np.diff(cand) <= 0):
            raise ValueError("candidates must be strictly increasing (sorted, no duplicates)")
        cand = np.ascontiguousarray(cand, dtype=np.int32)
    return n, kappa, cand


class PPCAModel:
    """Immutable PPCA model (ppca_model.rs:18-48; src/python_bindings.rs:367-533).

    y = C x + mean + noise, x ~ N(0, I), noise ~ N(0, isotropic_noise^2 I).
    """

    def __init__(self, isotropic_noise: float, transform, mean, *, ctx=None):
        t = np.array(transform, dtype=np.float64, order="C")
        if t.ndim != 2:
            raise TypeError("transform must be a 2-D float64 array (d, k)")
        m = np.asarray(mean, dtype=np.float64)
        if m.ndim == 2 and 1 in m.shape:
            m = m.reshape(-1)
        elif m.ndim == 2:
            # to_nalgebra_vector panics: "Expected column- or row- vector" (src/utils.rs:16-22)
            raise ValueError(f"Expected column- or row- vector; got {m.shape[0]}x{m.shape[1]} matrix")
        elif m.ndim != 1:
            raise TypeError("mean must be a vector")
        if m.shape[0] != t.shape[0]:
            raise ValueError("mean and transform disagree on the output size")
        self._sigma = float(isotropic_noise)
        self._c = t
        self._mean = np.array(m, dtype=np.float64)
        self._c.setflags(write=False)
        self._mean.setflags(write=False)
        self._ctx = ctx
        self._dev: Optional[_DevModel] = None

    # -- device handle ------------------------------------------------------
    def _device(self, ctx) -> _DevModel:
        if self._dev is None or self._dev_ctx is not ctx:
            h = C.c_void_p()
            check(lib().ppca_model_create(ctx.handle, self.output_size, self.state_size, self._sigma, ptr(self._c),
                                          ptr(self._mean), C.byref(h)))
            self._dev, self._dev_ctx = _DevModel(h), ctx
        return self._dev

    @classmethod
    def _from_device(cls, dev: _DevModel, ctx, d: int, k: int) -> "PPCAModel":
        sig = C.c_double(0.0)
        c = np.empty((d, k))
        m = np.empty(d)
        check(lib().ppca_model_download(dev.h, C.byref(sig), ptr(c), ptr(m)))
        out = cls(sig.value, c, m)
        out._dev, out._dev_ctx = dev, ctx
        return out

    # -- getters (src/python_bindings.rs:403-447) ------------------------------
    @property
    def output_size(self) -> int:
        return int(self._c.shape[0])

    @property
    def state_size(self) -> int:
        return int(self._c.shape[1])

    @property
    def n_parameters(self) -> int:
        """ppca_model.rs:107-109"""
        return 1 + self.state_size * self.output_size + self.output_size

    @property
    def singular_values(self) -> np.ndarray:
        """sqrt of each column's norm (sic, ppca_model.rs:113-121)."""
        return np.sqrt(np.linalg.norm(self._c, axis=0))

    @property
    def transform(self) -> np.ndarray:
        return self._c.copy()

    @property
    def isotropic_noise(self) -> float:
        return self._sigma

    @property
    def mean(self) -> np.ndarray:
        return self._mean.copy()

    def __repr__(self) -> str:  # shape of src/python_bindings.rs:454-464
        return (f"PPCAModel(isotropic_noise={self._sigma}, transform=array({self._c}, dtype=\"float64\"), "
                f"mean=narray({self._mean}, dtype=\"float64\"))")

    # -- construction ---------------------------------------------------------
    @staticmethod
    def init(state_size: int, dataset: Dataset, seed: Optional[int] = None, method: str = "random") -> "PPCAModel":
        """Random untrained model (ppca_model.rs:51-70): C ~ N(0,1) with the rows of
        all-masked dimensions zeroed, sigma = 1, mean = 0.  `seed` is an extension
        (the reference's RNG cannot be seeded).  method="pca" (an extension): the spectral start
        `from_moments(state_size, dataset.pairwise_moments())` instead; `seed` is not used.

        LIMIT: state_size <= 64.  The reference takes any state size; here the per-sample k x k inversion is one
        wave's job (a 64 x 64 matrix in 33 KB of LDS, ppca_generic.hip::solve_mfma_kernel) and the M-step row solves
        keep one row per lane.  Larger state sizes raise here instead of at the first kernel launch."""
        if len(dataset) == 0:
            raise ValueError("dataset is empty")  # assert!(!dataset.is_empty()) :52
        if state_size > 64:
            raise ValueError(f"state_size {state_size} is not supported: the MI355X kernels cover state sizes up to 64")
        if state_size < 0:
            raise ValueError("state_size must be >= 0")
        # state_size = 0 (an isotropic Gaussian around the mean, ppca_model.rs:51-70 with an empty transform; to_canonical
        # :399-402) is accepted as the reference accepts it: the library carries it as ONE zero transform column, with
        # which every pass reproduces the k = 0 model exactly (include/ppca_hip.h, ppca_model_create)
        if method == "pca":
            if isinstance(dataset, SparseDataset):
                raise ValueError("method='pca' is not available on a SparseDataset: the d x d moments are not built from row-compressed data")
            return PPCAModel.from_moments(state_size, dataset.pairwise_moments())
        if method != "random":
            raise ValueError("method must be 'random' or 'pca'")
        d = dataset.output_size()
        rng = np.random.default_rng(seed)
        # DMatrix::from_vec is column-major (utils.rs:16-25)
        c = rng.standard_normal(d * state_size).reshape((state_size, d)).T.copy()
        for j in dataset.empty_dimensions():
            c[j, :] = 0.0
        return PPCAModel(1.0, c, np.zeros(d))

    @staticmethod
    def from_moments(state_size: int, moments: "PairwiseMoments") -> "PPCAModel":
        """The spectral start: the closed-form maximum-likelihood PPCA model (Tipping and Bishop 1999) of the covariance
        sums / counts of `moments` (NaN -> 0) on the columns with an observed entry -- the top state_size eigenpairs (U, lambda),
        sigma^2 = the mean of the other eigenvalues (at least 1e-8 of the mean variance), C = U sqrt(max(lambda - sigma^2, 0)), zero
        rows on empty columns, mean = the centre; canonical, so the signs are determined.  With complete data it is a fixed point of
        EM; with masked data it is the standard start.  sigma = 1, C = 0 when the data has no variance.  Host-side numpy."""
        k = int(state_size)
        if k < 0:
            raise ValueError("state_size must be >= 0")
        counts = moments._counts
        sigma, c = _spectral_start(moments.covariance("global", 0.0), np.diag(counts) > 0.0, k)
        return PPCAModel(sigma, PPCAModel._canonical_transform(c), moments._center)

    @staticmethod
    def _canonical_transform(c: np.ndarray) -> np.ndarray:
        """The transform of to_canonical at the same state size: the SVD of a d x k matrix with k > d has d columns, the rest are 0."""
        out = np.zeros_like(c)
        t = PPCAModel(1.0, c, np.zeros(c.shape[0])).to_canonical()._c
        out[:, :t.shape[1]] = t
        return out

    def sample(self, dataset_size: int, mask_prob: float, seed: Optional[int] = None, *, ctx=None) -> Dataset:
        """ppca_model.rs:186-191, generated on the GPU with a counter-based RNG."""
        if not (0.0 <= mask_prob <= 1.0):
            raise ValueError("invalid mask probability")  # :171
        c = _ctx(ctx or self._ctx)
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        spec = _lib.SynthSpec(0, dataset_size, self.output_size, self.state_size, self._sigma, float(mask_prob), 0, 0,
                              seed, self._c.ctypes.data_as(_lib.c_double_p), self._mean.ctypes.data_as(_lib.c_double_p))
        h = C.c_void_p()
        check(lib().ppca_dataset_generate(c.handle, C.byref(spec), C.byref(h)))
        return Dataset._wrap(h, c)

    # -- hot path ---------------------------------------------------------------
    def llk(self, dataset: Dataset) -> float:
        """Weighted log-likelihood (ppca_model.rs:142-149)."""
        tot = C.c_double(0.0)
        if isinstance(dataset, SparseDataset):
            check(lib().ppca_sparse_llk(dataset._ctx.handle, dataset._sh, self._device(dataset._ctx).h, C.byref(tot), None))
            return tot.value
        check(lib().ppca_llk(dataset._ctx.handle, dataset._h, self._device(dataset._ctx).h, C.byref(tot), None))
        return tot.value

    def llks(self, dataset: Dataset) -> np.ndarray:
        """Per-sample log-likelihood (ppca_model.rs:152-159)."""
        out = np.empty(len(dataset))
        if isinstance(dataset, SparseDataset):
            check(lib().ppca_sparse_llk(dataset._ctx.handle, dataset._sh, self._device(dataset._ctx).h, None, ptr(out)))
            return out
        check(lib().ppca_llk(dataset._ctx.handle, dataset._h, self._device(dataset._ctx).h, None, ptr(out)))
        return out

    def infer(self, dataset: Dataset) -> "InferredMasked":
        """ppca_model.rs:221-227"""
        n, k = len(dataset), self.state_size
        states = np.empty((n, k))
        covs = np.empty((n, k, k))
        fn, h = (lib().ppca_sparse_infer, dataset._sh) if isinstance(dataset, SparseDataset) else (lib().ppca_infer, dataset._h)
        check(fn(dataset._ctx.handle, h, self._device(dataset._ctx).h, ptr(states), ptr(covs)))
        return InferredMasked(self, states, covs)

    def predict(self, sparse: "SparseDataset", query):
        """The predictive of a new reading at chosen positions of row-compressed data: `query` is a SparseDataset (its values are
        ignored) or an (indptr, indices) pair with the rows of `sparse`.  Returns (mean, var), one value per query entry in query
        order: mean = mean_j + c_j . z_i and var = c_j^T Sigma_i c_j + sigma^2 with (z_i, Sigma_i) the row's posterior given its
        entries in `sparse` -- the convention of `heldout_score`.  No N x d array is formed."""
        if not isinstance(sparse, SparseDataset):
            raise TypeError("predict takes a SparseDataset (on a Dataset: smooth / extrapolate / heldout_score)")
        ip, ix = _query_pattern(sparse, query)
        mean, var = np.empty(ix.size), np.empty(ix.size)
        ctx = sparse._ctx
        check(lib().ppca_sparse_predict(ctx.handle, sparse._sh, self._device(ctx).h, ptr(ip), ptr(ix), ptr(mean), ptr(var)))
        return mean, var

    def recommend(self, sparse: "SparseDataset", n: int, *, kappa: float = 0.0, exclude_observed: bool = True, candidates=None):
        """For every row of row-compressed data the n columns the model ranks highest, in one device pass.  The score
        of column j for row i is mean_ij + kappa sqrt(var_ij) with exactly `predict`'s two values: kappa = 0 ranks by the predictive
        mean, kappa > 0 by an upper confidence bound (exploration), kappa < 0 by a lower one.  Ranked are the row's candidate columns
        -- `candidates` (a strictly increasing int array of columns, e.g. the items in stock; None: all), without the columns the row has
        an entry in unless exclude_observed=False -- by score descending, equal scores by ascending column.  Returns (columns int32
        (N, n), scores float64 (N, n)); a row with fewer than n candidates is padded at the end with -1 and NaN.  1 <= n <= 64.  Row
        weights play no part, an empty row ranks with z = 0, Sigma = I, and no N x d array is formed.  Rows are independent: a shard
        calls this on its own rows."""
        n, kappa, cand = _recommend_args(sparse, n, kappa, candidates)
        if self.output_size != sparse._d:
            raise ValueError(f"dataset has {sparse._d} columns but the model has output size {self.output_size}")
        if self.state_size > 16:  # (the library's own answer, given here so that it comes before the first touch of a device)
            raise _lib.PPCAError(-3, f"state size {self.state_size} is not supported on sparse data: the kernels cover k <= 16")
        cols, scores = np.empty((len(sparse), n), dtype=np.int32), np.empty((len(sparse), n))
        if len(sparse) == 0:
            return cols, scores
        ctx = sparse._ctx
        cbuf = cand if cand is None or cand.size else np.zeros(1, dtype=np.int32)  # (an empty list is not NULL = every column)
        check(lib().ppca_topn_sparse(ctx.handle, sparse._sh, self._device(ctx).h, n, kappa, 1 if exclude_observed else 0, ptr(cbuf),
                                     0 if cand is None else cand.size, ptr(cols), ptr(scores)))
        return cols, scores

    @staticmethod
    def _recon_check(dataset: Dataset) -> None:
        if isinstance(dataset, SparseDataset):
            raise TypeError("smooth / extrapolate would write an N x d output, which is what a SparseDataset exists to avoid: use "
                            "predict(sparse, query) at the positions that are wanted")

    def _recon(self, dataset: Dataset, mode: int, fn) -> Dataset:
        self._recon_check(dataset)
        h = C.c_void_p()
        check(fn(dataset._ctx.handle, dataset._h, self._device(dataset._ctx).h, mode, C.byref(h)))
        return Dataset._wrap(h, dataset._ctx)

    def smooth(self, dataset: Dataset) -> Dataset:
        """C z + mean for every dimension (ppca_model.rs:237-244)."""
        return self._recon(dataset, 0, lib().ppca_reconstruct)

    filter_extrapolate = smooth  # README name (readme.md:62)

    def extrapolate(self, dataset: Dataset) -> Dataset:
        """Observed values kept, masked ones replaced by C z + mean (ppca_model.rs:254-261)."""
        return self._recon(dataset, 1, lib().ppca_reconstruct)

    def sample_posterior(self, dataset: Dataset, seed: Optional[int] = None, *, keep_observed: bool = False,
                         row_offset: int = 0) -> Dataset:
        """One draw per row from the posterior predictive, on the GPU in one pass: C (z + U eps) + mean + sigma eta with
        z, Sigma = U U^T the row's posterior (what `infer` returns) and eps, eta standard normals of a counter-based
        generator keyed by (seed, row_offset + row, index).  keep_observed=True: observed entries are passed through
        unchanged and only the masked ones are drawn (one draw of multiple imputation).  The result carries the input
        weights.  The draw of a row does not depend on how the dataset is split: a slice starting at row s with
        row_offset=s reproduces those rows of the whole.  seed=None draws a fresh seed."""
        if row_offset < 0:
            raise ValueError("row_offset must be >= 0")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        ctx = dataset._ctx
        h = C.c_void_p()
        check(lib().ppca_posterior_sample(ctx.handle, dataset._h, self._device(ctx).h, int(bool(keep_observed)),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), C.byref(h)))
        return Dataset._wrap(h, ctx)

    def _loo(self, dataset: Dataset, full: bool, per_sample: bool):
        ctx = dataset._ctx
        return _loo_call(dataset, full, per_sample, lambda mh, vh, tot, ps: lib().ppca_loo_predictive(
            ctx.handle, dataset._h, self._device(ctx).h, mh, vh, tot, ps))

    def loo_predictive(self, dataset: Dataset) -> "LooPredictive":
        """The predictive of every entry given the OTHER observed entries of its row, the model held fixed (one GPU pass; an
        extension with no reference counterpart).  Observed entries: the leave-one-out mean and variance, and the log-density
        of the entry under them; masked entries: the `extrapolate` value and the extrapolated covariance diagonal."""
        return self._loo(dataset, True, True)

    def loo_llks(self, dataset: Dataset) -> np.ndarray:
        """Per row, the sum over its observed entries of the leave-one-out log-density (0 for a row with none); no N x d output
        is written."""
        return self._loo(dataset, False, True)._llks

    def loo_llk(self, dataset: Dataset) -> float:
        """sum_i w_i loo_llks[i]: the leave-one-out pseudo-log-likelihood, a criterion for the state size that needs no refit."""
        return self._loo(dataset, False, False)._llk

    def heldout_score(self, train: Dataset, held: Dataset) -> "HeldOutScore":
        """How this model predicts the finite entries of `held` from the rows of `train` (the two parts of Dataset.holdout; any two
        datasets of one shape will do): per entry the predictive N(mean_j + c_j^T z, sigma^2 + c_j^T Sigma c_j) of a new reading
        of column j under the row's posterior (z, Sigma) given `train`.  One GPU pass over each dataset; no N x d output.
        Two SparseDatasets (the parts of SparseDataset.holdout) are scored the same way from their entry lists; they
        need one block_rows.  A Dataset with a SparseDataset raises TypeError."""
        sparse = isinstance(train, SparseDataset), isinstance(held, SparseDataset)
        if sparse[0] != sparse[1]:
            raise TypeError("heldout_score takes two Datasets or two SparseDatasets, not one of each")
        if sparse[0]:  # (the checks come before the first touch of a device)
            if len(train) == len(held) and train._d == held._d and train._block_rows != held._block_rows:
                raise ValueError(f"the train part is tiled with block_rows={train._block_rows or None} and the held part with "
                                 f"block_rows={held._block_rows or None}: the score walks both block by block, so build them with one "
                                 "block_rows tiling")
            return _heldout_call(train, held, lambda t, c, r: lib().ppca_heldout_score_sparse(
                train._ctx.handle, train._sh, held._sh, self._device(train._ctx).h, t, c, r))
        ctx = train._ctx
        return _heldout_call(train, held, lambda t, c, r: lib().ppca_heldout_score(ctx.handle, train._h, held._h, self._device(ctx).h,
                                                                                  t, c, r))

    def _iterate(self, dataset: Dataset, prior: Optional[Prior], want_llk: bool):
        ctx = dataset._ctx
        if len(dataset) == 0:
            raise ValueError("dataset is empty")
        out = C.c_void_p()
        check(lib().ppca_model_alloc(ctx.handle, self.output_size, self.state_size, C.byref(out)))
        dev_out = _DevModel(out)
        pref, keep = _prior_ref(prior)
        llk = C.c_double(0.0)
        fn, h = (lib().ppca_sparse_em_step, dataset._sh) if isinstance(dataset, SparseDataset) else (lib().ppca_em_step, dataset._h)
        check(fn(ctx.handle, h, self._device(ctx).h, pref, dev_out.h, C.byref(llk) if want_llk else None))
        new = PPCAModel._from_device(dev_out, ctx, self.output_size, self.state_size)
        return new, (llk.value if want_llk else None)

    def iterate(self, dataset: Dataset) -> "PPCAModel":
        """One EM iteration (ppca_model.rs:267-269)."""
        return self._iterate(dataset, None, False)[0]

    def iterate_with_prior(self, dataset: Dataset, prior: Prior) -> "PPCAModel":
        """One MAP-EM iteration (ppca_model.rs:277-393)."""
        return self._iterate(dataset, prior, False)[0]

    def iterate_with_llk(self, dataset: Dataset, prior: Optional[Prior] = None):
        """Extension: (next model, llk of THIS model) from the same single pass."""
        return self._iterate(dataset, prior, True)

    def to_canonical(self) -> "PPCAModel":
        """C = U S V^T -> U S, columns by descending singular value, sign = signum(column sum)
        (ppca_model.rs:398-425).  Host-side, O(d k^2)."""
        if self.state_size == 0:
            return self
        u, s, _ = np.linalg.svd(self._c, full_matrices=False)
        c = u * s
        sums = c.sum(axis=0)
        c = c * np.where(np.signbit(sums), -1.0, 1.0)
        return PPCAModel(self._sigma, c, self._mean)

    # -- serialisation (own container; bincode layout is a "next" row) ------------
    def dump(self, format: str = "npz") -> bytes:
        """src/python_bindings.rs:394-401; format="bincode": the reference's layout (wire.py, parity unpinned)."""
        if format == "bincode":
            return _wire.dump_model(self._sigma, self._c, self._mean)
        buf = io.BytesIO()
        np.savez(buf, kind="ppca_rs_amd.PPCAModel", isotropic_noise=self._sigma, transform=self._c, mean=self._mean)
        return buf.getvalue()

    @staticmethod
    def load(data: bytes) -> "PPCAModel":
        try:
            if bytes(data[:2]) != b"PK":
                return PPCAModel(*_wire.load_model(data))
            z = np.load(io.BytesIO(data), allow_pickle=False)
            return PPCAModel(float(z["isotropic_noise"]), z["transform"], z["mean"])
        except Exception as err:
            raise Exception(str(err))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        o = PPCAModel.load(state)
        self.__dict__.update(o.__dict__)

    def __getnewargs__(self):
        return (self._sigma, self.transform, self.mean)


# --------------------------------------------------------------------------- InferredMasked
class InferredMasked:
    """Batch of per-sample posteriors (src/python_bindings.rs:203-345; ppca_model.rs:430-593)."""

    def __init__(self, model: PPCAModel, states: np.ndarray, covs: np.ndarray):
        self._model, self._states, self._covs = model, states, covs

    def states(self) -> np.ndarray:
        if self._states.shape[0] == 0:
            return np.zeros((0, 0))
        return self._states.copy()

    def covariances(self) -> List[np.ndarray]:
        return [c.copy() for c in self._covs]

    def _as_dataset(self, arr: np.ndarray) -> Dataset:
        return Dataset(np.ascontiguousarray(arr))

    def smoothed(self, ppca: PPCAModel) -> Dataset:
        """C z + mean (ppca_model.rs:454-456)."""
        return self._as_dataset(self._states @ ppca._c.T + ppca._mean)

    def extrapolated(self, ppca: PPCAModel, dataset: Dataset) -> Dataset:
        """ppca_model.rs:460-463"""
        x = dataset.numpy()
        sm = self._states @ ppca._c.T + ppca._mean
        return self._as_dataset(np.where(np.isfinite(x), x, sm))

    def smoothed_covariances(self, ppca: PPCAModel) -> List[np.ndarray]:
        """sigma^2 I + C Sigma C^T per sample (ppca_model.rs:471-477) -- d x d each."""
        d = ppca.output_size
        eye = np.eye(d) * ppca._sigma ** 2
        return [eye + ppca._c @ cv @ ppca._c.T for cv in self._covs]

    def smoothed_covariances_diagonal(self, ppca: PPCAModel) -> Dataset:
        """ppca_model.rs:485-508"""
        diag = np.einsum("ja,nab,jb->nj", ppca._c, self._covs, ppca._c) + ppca._sigma ** 2
        return self._as_dataset(diag)

    def extrapolated_covariances(self, ppca: PPCAModel, dataset: Dataset) -> List[np.ndarray]:
        """ppca_model.rs:517-534"""
        x = dataset.numpy()
        d = ppca.output_size
        out = []
        for cv, row in zip(self._covs, x):
            neg = ~np.isfinite(row)
            full = np.zeros((d, d))
            if neg.any():
                cn = ppca._c[neg]
                full[np.ix_(neg, neg)] = np.eye(neg.sum()) * ppca._sigma ** 2 + cn @ cv @ cn.T
            out.append(full)
        return out

    def extrapolated_covariances_diagonal(self, ppca: PPCAModel, dataset: Dataset) -> Dataset:
        """ppca_model.rs:542-577"""
        x = dataset.numpy()
        diag = np.einsum("ja,nab,jb->nj", ppca._c, self._covs, ppca._c) + ppca._sigma ** 2
        return self._as_dataset(np.where(np.isfinite(x), 0.0, diag))

    def posterior_sampler(self) -> "PosteriorSampler":
        """ppca_model.rs:581-592 -- host-side, with numpy's generator (its draws for a seed are kept as they are).
        PPCAModel.sample_posterior draws on the GPU in one pass, without the covariances leaving the device."""
        return PosteriorSampler(self._model, self._states, np.linalg.cholesky(self._covs))


def _loo_call(dataset: Dataset, full: bool, per_sample: bool, fn) -> "LooPredictive":
    ctx = dataset._ctx
    mh, vh = C.c_void_p(), C.c_void_p()
    tot = C.c_double(0.0)
    llks = np.empty(len(dataset)) if per_sample else None
    check(fn(C.byref(mh) if full else None, C.byref(vh) if full else None, C.byref(tot), ptr(llks)))
    mean = Dataset._wrap(mh, ctx) if full else None
    var = Dataset._wrap(vh, ctx) if full else None
    return LooPredictive(dataset, mean, var, llks, tot.value)


class LooPredictive:
    """What PPCAModel.loo_predictive / PPCAMix.loo_predictive return: per entry the predictive given the other observed
    entries of the row (mean(), variance(): device-resident datasets), per row the sum of the observed entries' log-densities
    (llks()) and its weighted total (llk())."""

    def __init__(self, dataset: Dataset, mean: Optional[Dataset], var: Optional[Dataset], llks: Optional[np.ndarray], llk: float):
        self._dataset, self._mean, self._var, self._llks, self._llk = dataset, mean, var, llks, llk

    def mean(self) -> Dataset:
        return self._mean

    def variance(self) -> Dataset:
        return self._var

    def llks(self) -> np.ndarray:
        return self._llks.copy()

    def llk(self) -> float:
        return self._llk

    def zscores(self) -> np.ndarray:
        """Host-side (x - mean) / sqrt(variance) on observed entries, NaN on masked ones: standard normal under a calibrated
        model; a large magnitude marks the entry of a row that its other entries do not explain."""
        x = self._dataset.numpy()
        z = (x - self._mean.numpy()) / np.sqrt(self._var.numpy())
        z[~np.isfinite(x)] = np.nan
        return z


class PosteriorSampler:
    """ppca_model.rs:597-626; src/python_bindings.rs:347-365.  Host-side; see PPCAModel.sample_posterior for the GPU pass."""

    def __init__(self, model: PPCAModel, states: np.ndarray, chol: np.ndarray):
        self._model, self._states, self._chol = model, states, chol

    def sample(self, seed: Optional[int] = None) -> Dataset:
        rng = np.random.default_rng(seed)
        n, k = self._states.shape
        m = self._model
        std = rng.standard_normal((n, k))
        noise = m._sigma * rng.standard_normal((n, m.output_size))
        z = self._states + np.einsum("nab,nb->na", self._chol, std)
        return Dataset(np.ascontiguousarray(noise + m._mean + z @ m._c.T))


# --------------------------------------------------------------------------- held-out scoring
class HeldOutScore:
    """What `heldout_score` returns: how a model fitted on the train part of Dataset.holdout predicts the held entries.

    count       sum_i w_i (held entries of row i)            n_entries   the unweighted entry count
    llk         sum w l, l the predictive log-density        mean_llk    llk / count
    mse, rmse   sum w e^2 / count and its root               mean_z2     sum w e^2 / v / count (about 1 when the intervals are calibrated)
    llks        per row, the sum of l over its held entries (0 for a row with none)
    columns     per column: count, llk, se (sum w e^2), z2 (sum w e^2 / v), rmse
    Scores of disjoint shards add (`a + b`): sums field by field, llks concatenated.  Scores of several folds of the same rows
    (Dataset.kfold) pool (`HeldOutScore.pooled`): sums field by field, llks added row by row."""

    def __init__(self, col_sums: np.ndarray, n_entries: float, n_rows: float, llks: np.ndarray):
        self._cols = np.asarray(col_sums, dtype=np.float64).reshape(4, -1)
        self.n_entries, self.n_rows, self._llks = int(n_entries), int(n_rows), np.asarray(llks, dtype=np.float64)
        self.count, self.llk, self._se, self._z2 = (float(sum(row.tolist())) for row in self._cols)  # (the columns in index order)

    @staticmethod
    def _ratio(a, b):
        return a / b if b > 0 else float("nan")

    @property
    def mean_llk(self) -> float:
        return self._ratio(self.llk, self.count)

    @property
    def mse(self) -> float:
        return self._ratio(self._se, self.count)

    @property
    def rmse(self) -> float:
        return math.sqrt(self.mse)

    @property
    def mean_z2(self) -> float:
        return self._ratio(self._z2, self.count)

    @property
    def llks(self) -> np.ndarray:
        return self._llks.copy()

    @property
    def columns(self) -> dict:
        cnt, llk, se, z2 = (row.copy() for row in self._cols)
        with np.errstate(invalid="ignore", divide="ignore"):
            rmse = np.sqrt(se / cnt)
        return dict(count=cnt, llk=llk, se=se, z2=z2, rmse=rmse)

    def __add__(self, other: "HeldOutScore") -> "HeldOutScore":
        if self._cols.shape != other._cols.shape:
            raise ValueError("the two scores are of different output sizes")
        return HeldOutScore(self._cols + other._cols, self.n_entries + other.n_entries, self.n_rows + other.n_rows,
                            np.concatenate([self._llks, other._llks]))

    @staticmethod
    def pooled(scores) -> "HeldOutScore":
        """The scores of several folds of the SAME rows (Dataset.kfold) as one: column sums and entry counts added, llks added row by
        row; n_rows adds too, so it counts (row, fold) pairs with a held entry.  `a + b` is for disjoint shards."""
        scores = list(scores)
        if not scores:
            raise ValueError("no scores to pool")
        first = scores[0]
        if any(s._cols.shape != first._cols.shape or s._llks.shape != first._llks.shape for s in scores):
            raise ValueError("the scores are of different shapes")
        cols, llks = first._cols.copy(), first._llks.copy()
        for s in scores[1:]:
            cols += s._cols
            llks += s._llks
        return HeldOutScore(cols, sum(s.n_entries for s in scores), sum(s.n_rows for s in scores), llks)

    def __repr__(self) -> str:
        return f"HeldOutScore(n_entries={self.n_entries}, mean_llk={self.mean_llk:.6g}, rmse={self.rmse:.6g}, mean_z2={self.mean_z2:.4g})"


def _heldout_call(train: Dataset, held: Dataset, fn) -> HeldOutScore:
    if len(train) != len(held) or train._d != held._d:
        raise ValueError("the train part and the held part differ in shape")
    totals, cols, rows = np.zeros(6), np.zeros((4, train._d)), np.zeros(len(train))
    check(fn(ptr(totals), ptr(cols), ptr(rows)))
    return HeldOutScore(cols, totals[4], totals[5], rows)


def _heldout_unwhiten(score: HeldOutScore, held: Dataset, noise: np.ndarray) -> HeldOutScore:
    """The score of whitened data (columns divided by noise) in the units of the data: llk_j -= cnt_j ln s_j, se_j *= s_j^2, z2_j
    unchanged; per row, minus the sum of ln s_j over the row's held entries."""
    ln = np.log(noise)
    _, _, jac = held._scale_columns(np.ones_like(noise), l=ln, out=False, row_sums=True)
    cols = score._cols.copy()
    cols[1] -= cols[0] * ln
    cols[2] *= noise * noise
    return HeldOutScore(cols, score.n_entries, score.n_rows, score._llks - jac)


def heldout_score(model, train: Dataset, held: Dataset, precisions=None, held_precisions=None) -> HeldOutScore:
    """The held-out score of a model of ANY family on one split, so that families are compared on identical held entries:
    model.heldout_score(train, held) for PPCAModel, PPCAMix, FAModel and FAMix; TPPCAModel.score_heldout(train, held) (the t
    predictive); HPPCAModel.score_heldout(train, held, precisions, held_precisions) (an entry at its own noise level).  `precisions`
    are required for an HPPCAModel and refused for every other family.  Two SparseDatasets are scored by a PPCAModel only (an FAModel
    scores them through its own method, FAModel.heldout_score: taking it here, and in cross_validate, is the follow-up of DESIGN.md 7)."""
    if (isinstance(train, SparseDataset) or isinstance(held, SparseDataset)) and not isinstance(model, PPCAModel):
        raise TypeError(f"{type(model).__name__} does not score a SparseDataset: on row-compressed data only PPCAModel.heldout_score exists "
                        "(DESIGN.md section 7)")
    if isinstance(model, HPPCAModel):
        if precisions is None:
            raise ValueError("an HPPCAModel is scored under precisions")
        return model.score_heldout(train, held, precisions, held_precisions)
    if precisions is not None or held_precisions is not None:
        raise ValueError(f"{type(model).__name__} takes no precisions")
    return model.score_heldout(train, held) if isinstance(model, TPPCAModel) else model.heldout_score(train, held)


def _select_state_size(dataset: Dataset, state_sizes, fraction: float, seed: Optional[int], fit, folds: int = 1, score=None):
    """One hold-out split, then per state size fit(train part, k) -> model and its score on the held part (score(model, train, held);
    default heldout_score(model, train, held)).  folds > 1: the split is dataset.kfold(folds, seed) instead (`fraction` is not used),
    one fit per size and fold; the score is HeldOutScore.pooled over the folds and the third element the list of the folds' models."""
    score = score or heldout_score
    if int(folds) < 1:
        raise ValueError("folds must be >= 1")
    if int(folds) == 1:
        train, held = dataset.holdout(fraction, seed)
        out = []
        for k in state_sizes:
            model = fit(train, int(k))
            out.append((int(k), score(model, train, held), model))
        return out
    parts = dataset.kfold(int(folds), seed)
    out = []
    for k in state_sizes:
        models = [fit(train, int(k)) for train, _ in parts]
        out.append((int(k), HeldOutScore.pooled([score(m, train, held) for m, (train, held) in zip(models, parts)]), models))
    return out


def cross_validate(dataset: Dataset, fit, *, folds: int = 5, seed: Optional[int] = None, precisions=None):
    """K-fold entry-wise cross-validation of any model family on the folds of dataset.kfold(folds, seed): per fold
    model = fit(train) -- fit(train, precisions) when `precisions` (a Dataset or an array of the dataset's shape) is given -- and
    heldout_score(model, train, held[, precisions]).  Returns (the folds' scores, HeldOutScore.pooled of them, the folds' models).
    The folds depend on (seed, shape) alone, so fits of different families with the same seed are compared on identical held
    entries.  `fit` may return the model or a tuple that starts with it (HPPCATrainer.train's (model, metrics)).  `dataset` may be a
    SparseDataset (the folds of SparseDataset.kfold, PPCAModel fits; no precisions)."""
    if isinstance(dataset, SparseDataset) and precisions is not None:
        raise ValueError("precisions are not available with a SparseDataset: the known-precision model takes a dense Dataset")
    if precisions is not None and not isinstance(precisions, Dataset):
        p = np.ascontiguousarray(precisions, dtype=np.float64)
        if p.shape != (len(dataset), dataset._d):
            raise ValueError(f"precisions have shape {p.shape} but the dataset is {len(dataset)} x {dataset._d}")
        precisions = Dataset(p, ctx=dataset._ctx)
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    scores, models = [], []
    for train, held in dataset.kfold(folds, seed):
        model = fit(train) if precisions is None else fit(train, precisions)
        model = model[0] if isinstance(model, tuple) else model
        scores.append(heldout_score(model, train, held, precisions))
        models.append(model)
    return scores, HeldOutScore.pooled(scores), models


# --------------------------------------------------------------------------- trainers
@dataclass(frozen=True)
class TrainMetrics:
    """python/ppca_rs/__init__.py:14-18"""
    llk: float
    aic: float
    bic: float


def _metrics(llk: float, n_parameters: int, n: int) -> TrainMetrics:
    # formulas as written in python/ppca_rs/__init__.py:52-57
    return TrainMetrics(llk=llk / n, aic=2.0 * (n_parameters - llk) / n, bic=(llk - n_parameters * np.log(n)) / n)


def _train_loop(model, n_iters: int, quiet: bool, metric: str, label: str, n: int, step_with_llk, step, n_parameters=None):
    """The loop of every trainer (python/ppca_rs/__init__.py:45-66).  step_with_llk(model) -> (next model, llk of `model`);
    step(model) -> next model, the quiet form, which reads no llk back; n_parameters(model): the count behind aic / bic where it is
    not model.n_parameters."""
    for idx in range(n_iters):
        if quiet:
            model = step(model)
            continue
        # the llk of the current model is a by-product of the EM pass: no second sweep
        new_model, llk = step_with_llk(model)
        metrics = _metrics(llk, n_parameters(model) if n_parameters else model.n_parameters, n)
        print(f"Masked {label} iteration {idx + 1}: {metric}={getattr(metrics, metric)}")
        model = new_model
    return model.to_canonical()


@dataclass
class PPCATrainer:
    """EM driver (python/ppca_rs/__init__.py:21-67)."""

    dataset: Dataset

    def train(self, *, start: Optional[PPCAModel] = None, prior: Optional[Prior] = None, state_size: int,
              n_iters: int = 10, metric: Literal["aic", "bic", "llk"] = "aic", quiet: bool = False,
              seed: Optional[int] = None, init: str = "random") -> PPCAModel:
        """init: the method of PPCAModel.init ("random" or "pca"), used only when `start` is None."""
        ds = self.dataset
        model = start or PPCAModel.init(state_size, ds, seed=seed, method=init)
        return _train_loop(model, n_iters, quiet, metric, "PPCA", len(ds), lambda m: m.iterate_with_llk(ds, prior),
                           lambda m: m.iterate_with_prior(ds, prior) if prior is not None else m.iterate(ds))


    def select_state_size(self, state_sizes, *, fraction: float = 0.1, seed: Optional[int] = None, n_iters: int = 10,
                          init: str = "random", prior: Optional[Prior] = None, folds: int = 1):
        """Entry-wise cross-validation of the state size: one Dataset.holdout(fraction, seed), then for every size one `train` on the
        train part (quiet; model seed = `seed`) and one `heldout_score`.  Returns [(state_size, HeldOutScore, PPCAModel)]: choose the
        size whose score.mean_llk is largest.  folds > 1: the split is Dataset.kfold(folds, seed) instead (`fraction` is not used),
        one fit per size and fold; the score is the pooled one and the third element the list of the folds' models.  On a
        SparseDataset the split is SparseDataset.holdout / kfold (the same entries as the dense split) and init="pca" raises."""
        return _select_state_size(self.dataset, state_sizes, fraction, seed, lambda tr, k: PPCATrainer(tr).train(
            state_size=k, n_iters=n_iters, quiet=True, seed=seed, init=init, prior=prior), folds)


# --------------------------------------------------------------------------- own npz containers (FAModel, TPPCAModel, FAMix)
def _npz_dump(kind: str, **arrays) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, kind=kind, **arrays)
    return buf.getvalue()


def _npz_load(data: bytes, kind: str, label: str, build):
    """build(the container's arrays) once its `kind` is the expected one; label: the class with its article, as the mismatch message
    names it.  Whatever fails on the way is raised as a plain Exception with that failure's text."""
    try:
        z = np.load(io.BytesIO(data), allow_pickle=False)
        if str(z["kind"]) != kind:
            raise ValueError(f"not {label} container: {z['kind']}")
        return build(z)
    except Exception as err:
        raise Exception(str(err))


# --------------------------------------------------------------------------- factor analysis (per-column noise)
class InferredFA:
    """What FAModel.infer returns: the per-sample posterior means and covariances of the latent state."""

    def __init__(self, states: np.ndarray, covs: np.ndarray):
        self._states, self._covs = states, covs

    def states(self) -> np.ndarray:
        if self._states.shape[0] == 0:
            return np.zeros((0, 0))
        return self._states.copy()

    def covariances(self) -> List[np.ndarray]:
        return [c.copy() for c in self._covs]


class FAModel:
    """Masked factor analysis: y = C x + mean + noise, x ~ N(0, I), noise_j ~ N(0, noise[j]^2) -- PPCAModel with one noise level
    per column (an extension with no reference counterpart; include/ppca_hip.h).

    Every pass runs the PPCA kernels on the dataset with column j divided by noise[j] (`whitened()` is the model of that
    dataset); the whitened copy is made on the GPU for the call and released with it: at most one is alive at a time.
    """

    def __init__(self, noise, transform, mean, *, ctx=None):
        base = PPCAModel(1.0, transform, mean, ctx=ctx)  # (the checks of transform and mean are PPCAModel's)
        n = np.array(noise, dtype=np.float64)
        if n.ndim != 1 or n.shape[0] != base.output_size:
            raise ValueError(f"noise must have shape ({base.output_size},): one level per column")
        if not (np.all(np.isfinite(n)) and np.all(n > 0.0)):
            raise ValueError("every entry of noise must be a positive finite number")
        self._noise, self._c, self._mean, self._ctx = n, base._c, base._mean, ctx
        self._noise.setflags(write=False)

    # -- getters ----------------------------------------------------------------
    @property
    def noise(self) -> np.ndarray:
        return self._noise.copy()

    @property
    def transform(self) -> np.ndarray:
        return self._c.copy()

    @property
    def mean(self) -> np.ndarray:
        return self._mean.copy()

    @property
    def output_size(self) -> int:
        return int(self._c.shape[0])

    @property
    def state_size(self) -> int:
        return int(self._c.shape[1])

    @property
    def n_parameters(self) -> int:
        return 2 * self.output_size + self.output_size * self.state_size

    def __repr__(self) -> str:
        return f"FAModel(noise=array({self._noise}), transform=array({self._c}), mean=array({self._mean}))"

    # -- construction -------------------------------------------------------------
    @staticmethod
    def init(state_size: int, dataset: Dataset, seed: Optional[int] = None, method: str = "random") -> "FAModel":
        """The transform of PPCAModel.init (same seed, same draw), noise = 1, mean = 0.  method="pca": the spectral start
        `from_moments(state_size, dataset.pairwise_moments())` instead."""
        if method not in ("random", "pca"):
            raise ValueError("method must be 'random' or 'pca'")
        m = PPCAModel.init(state_size, dataset, seed=seed)  # (the checks of state_size and of an empty dataset, for both methods)
        if method == "pca":
            if isinstance(dataset, SparseDataset):
                raise ValueError("method='pca' is not available on a SparseDataset: the d x d moments are not built from row-compressed data")
            return FAModel.from_moments(state_size, dataset.pairwise_moments())
        return FAModel(np.ones(m.output_size), m._c, m._mean)

    @staticmethod
    def from_moments(state_size: int, moments: "PairwiseMoments") -> "FAModel":
        """The spectral start of factor analysis: the closed form of PPCAModel.from_moments on the CORRELATION matrix (C_r, with
        sd_j = sqrt(cov_jj), 1 where that is not positive), then C = diag(sd) C_r, noise_j = sd_j sqrt(max(1 - |C_r,j|^2, 1e-4))
        (1 for an empty column) and mean = the centre.  Rescaling a column rescales its row of C, its noise and its mean with it."""
        k = int(state_size)
        if k < 0:
            raise ValueError("state_size must be >= 0")
        cov = np.nan_to_num(moments.covariance("global", 0.0), nan=0.0, posinf=0.0, neginf=0.0)
        live = np.diag(moments._counts) > 0.0
        var = np.diag(cov)
        sd = np.where(var > 0.0, np.sqrt(np.where(var > 0.0, var, 1.0)), 1.0)
        _, c_r = _spectral_start(cov / np.outer(sd, sd), live, k)
        c_r = PPCAModel._canonical_transform(c_r)  # (signs and order fixed BEFORE the columns get their scale back)
        noise = np.where(live, sd * np.sqrt(np.maximum(1.0 - np.sum(c_r * c_r, axis=1), 1e-4)), 1.0)
        return FAModel(noise, sd[:, None] * c_r, moments._center)

    @staticmethod
    def from_ppca(model: PPCAModel) -> "FAModel":
        """The FA model equal to an isotropic one: noise = sigma on every column."""
        return FAModel(np.full(model.output_size, model.isotropic_noise), model._c, model._mean)

    def whitened(self) -> PPCAModel:
        """PPCAModel(1, diag(1 / noise) C, mean / noise): the model of the dataset whose column j is divided by noise[j]."""
        return PPCAModel(1.0, self._c / self._noise[:, None], self._mean / self._noise, ctx=self._ctx)

    def to_canonical(self) -> "FAModel":
        """The rotation of PPCAModel.to_canonical on C; noise and mean are untouched."""
        return FAModel(self._noise, PPCAModel(1.0, self._c, self._mean).to_canonical()._c, self._mean)

    def sample(self, dataset_size: int, mask_prob: float, seed: Optional[int] = None, *, ctx=None) -> Dataset:
        """The whitened model's `sample` (generated on the GPU) with column j multiplied by noise[j]."""
        white = self.whitened().sample(dataset_size, mask_prob, seed, ctx=ctx or self._ctx)
        return white._scale_columns(self._noise)[0]

    # -- passes ---------------------------------------------------------------------
    def _whiten(self, dataset: Dataset, **kw):
        if dataset._d != self.output_size:
            raise ValueError(f"dataset has {dataset._d} dimensions but the model has output size {self.output_size}")
        if isinstance(dataset, SparseDataset) and self.state_size > 16:  # (the library's own answer, before the first touch of a device)
            raise _lib.PPCAError(-3, f"state size {self.state_size} is not supported on sparse data: the kernels cover k <= 16")
        return dataset._scale_columns(1.0 / self._noise, **kw)

    def llks(self, dataset: Dataset) -> np.ndarray:
        """Per-sample log-likelihood: the whitened model's on the whitened rows minus the sum of ln noise[j] over the row's
        observed entries.  A SparseDataset is whitened on the device as a values view, here and in every pass below."""
        y, _, jac = self._whiten(dataset, l=np.log(self._noise), row_sums=True)
        return self.whitened().llks(y) - jac

    def llk(self, dataset: Dataset) -> float:
        """Weighted log-likelihood."""
        y, sums, _ = self._whiten(dataset, col_sums=True)
        return self.whitened().llk(y) - float(np.dot(sums[0], np.log(self._noise)))

    def heldout_score(self, train: Dataset, held: Dataset) -> "HeldOutScore":
        """PPCAModel.heldout_score for per-column noise: both parts whitened with the same scales, scored by the whitened model and
        mapped back to the units of the data.  Two SparseDatasets (the parts of SparseDataset.holdout) are whitened on the device as
        values views and scored from their entry lists; the one-of-each and block_rows checks are PPCAModel's.  (The
        package-level heldout_score(model, sparse, sparse) and cross_validate still take a PPCAModel only: DESIGN.md section 7.)"""
        sparse = isinstance(train, SparseDataset), isinstance(held, SparseDataset)
        if sparse[0] != sparse[1]:
            raise TypeError("heldout_score takes two Datasets or two SparseDatasets, not one of each")
        if sparse[0]:  # (PPCAModel.heldout_score's checks, before the first touch of a device)
            if len(train) == len(held) and train._d == held._d and train._block_rows != held._block_rows:
                raise ValueError(f"the train part is tiled with block_rows={train._block_rows or None} and the held part with "
                                 f"block_rows={held._block_rows or None}: the score walks both block by block, so build them with one "
                                 "block_rows tiling")
            if len(train) != len(held) or train._d != held._d:
                raise ValueError("the train part and the held part differ in shape")
        score = self.whitened().heldout_score(self._whiten(train)[0], self._whiten(held)[0])
        return _heldout_unwhiten(score, held, self._noise)

    def infer(self, dataset: Dataset) -> InferredFA:
        """Posterior of the latent state of every sample (that of the whitened model on the whitened rows)."""
        inf = self.whitened().infer(self._whiten(dataset)[0])
        return InferredFA(inf._states, inf._covs)

    def predict(self, sparse: "SparseDataset", query):
        """PPCAModel.predict for per-column noise: (mean, variance) of a new reading at the query positions of row-compressed data, in
        the units of the data -- the whitened model's predict on the whitened view, the mean times noise[j] and the variance times
        noise[j]^2."""
        if not isinstance(sparse, SparseDataset):
            raise TypeError("predict takes a SparseDataset (on a Dataset: smooth / extrapolate / heldout_score)")
        _, ix = _query_pattern(sparse, query)
        mean, var = self.whitened().predict(self._whiten(sparse)[0], query)
        s = self._noise[ix]
        return mean * s, var * (s * s)

    def smooth(self, dataset: Dataset) -> Dataset:
        """C z + mean for every dimension."""
        PPCAModel._recon_check(dataset)
        sm = self.whitened().smooth(self._whiten(dataset)[0])  # (the whitened copy is released here)
        return sm._scale_columns(self._noise)[0]

    def extrapolate(self, dataset: Dataset) -> Dataset:
        """Observed values kept bit for bit, masked ones replaced by C z + mean."""
        PPCAModel._recon_check(dataset)
        sm = self.whitened().smooth(self._whiten(dataset)[0])
        return dataset._fill_masked(sm, self._noise)

    def _iterate(self, dataset: Dataset, min_noise, want_llk: bool):
        if len(dataset) == 0:
            raise ValueError("dataset is empty")
        d, k = self.output_size, self.state_size
        if dataset._d != d:
            raise ValueError(f"dataset has {dataset._d} dimensions but the model has output size {d}")
        floor = None
        if min_noise is not None:
            floor = np.ascontiguousarray(np.broadcast_to(np.asarray(min_noise, dtype=np.float64), (d,)))
        n_out, c_out, m_out = np.empty(d), np.empty((d, k)), np.empty(d)
        llk = C.c_double(0.0)
        if isinstance(dataset, SparseDataset):
            if k > 16:  # (the library's own answer, given here so that it comes before the first touch of a device)
                raise _lib.PPCAError(-3, f"state size {k} is not supported on sparse data: the kernels cover k <= 16")
            fn, h = lib().ppca_fa_sparse_em_step, dataset._sh
        else:
            fn, h = lib().ppca_fa_em_step, dataset._h
        check(fn(dataset._ctx.handle, h, d, k, ptr(self._noise), ptr(self._c), ptr(self._mean), ptr(floor),
                 ptr(n_out), ptr(c_out), ptr(m_out), C.byref(llk) if want_llk else None))
        return FAModel(n_out, c_out, m_out, ctx=self._ctx), (llk.value if want_llk else None)

    def iterate(self, dataset: Dataset, min_noise=None) -> "FAModel":
        """One ECM iteration (transform, then mean, then noise, each given the ones before it: the log-likelihood cannot
        decrease).  min_noise: a floor for the new noise, a number or one per column."""
        return self._iterate(dataset, min_noise, False)[0]

    def iterate_with_llk(self, dataset: Dataset, min_noise=None):
        """(next model, llk of THIS model) from the same pass."""
        return self._iterate(dataset, min_noise, True)

    # -- serialisation (own npz container) ----------------------------------------------
    def dump(self) -> bytes:
        return _npz_dump("ppca_rs_amd.FAModel", noise=self._noise, transform=self._c, mean=self._mean)

    @staticmethod
    def load(data: bytes) -> "FAModel":
        return _npz_load(data, "ppca_rs_amd.FAModel", "an FAModel", lambda z: FAModel(z["noise"], z["transform"], z["mean"]))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        self.__dict__.update(FAModel.load(state).__dict__)

    def __getnewargs__(self):
        return (self.noise, self.transform, self.mean)


@dataclass
class FATrainer:
    """EM driver of FAModel: the loop and metrics of PPCATrainer."""

    dataset: Dataset

    def train(self, *, state_size: int, n_iters: int = 10, start: Optional[FAModel] = None,
              metric: Literal["aic", "bic", "llk"] = "aic", quiet: bool = False, seed: Optional[int] = None,
              min_noise_ratio: float = 1e-3, init: str = "random") -> FAModel:
        """init: the method of FAModel.init ("random" or "pca"), used only when `start` is None.
        min_noise_ratio: the new noise of column j is kept at or above ratio x the column's observed standard deviation -- a guard
        against a noise level collapsing to 0 (a Heywood case), not a tuned number: at 1e-3 it bounds the share of a column's
        variance the latent state may explain at 1 - 1e-6."""
        ds = self.dataset
        model = start or FAModel.init(state_size, ds, seed=seed, method=init)
        floor = min_noise_ratio * np.sqrt(ds.column_stats()[2])
        return _train_loop(model, n_iters, quiet, metric, "FA", len(ds), lambda m: m.iterate_with_llk(ds, floor),
                           lambda m: m.iterate(ds, floor))


    def select_state_size(self, state_sizes, *, fraction: float = 0.1, seed: Optional[int] = None, n_iters: int = 10,
                          init: str = "random", prior: Optional[Prior] = None, folds: int = 1):
        """PPCATrainer.select_state_size with FAModel fits: [(state_size, HeldOutScore, FAModel)].  FAModel has no MAP step:
        `prior` must be None.  On a SparseDataset the split is SparseDataset.holdout / kfold and the score FAModel.heldout_score on
        the two parts (the package-level heldout_score does not take an FAModel with row-compressed data)."""
        if prior is not None:
            raise ValueError("FATrainer takes no prior")
        return _select_state_size(self.dataset, state_sizes, fraction, seed, lambda tr, k: FATrainer(tr).train(
            state_size=k, n_iters=n_iters, quiet=True, seed=seed, init=init), folds, score=lambda m, t, h: m.heldout_score(t, h))


# --------------------------------------------------------------------------- Student-t PPCA (robust to outlying rows)
def _t_tables(d: int, dof: float):
    lg, g = np.empty(d + 1), np.empty(d + 1)
    check(lib().ppca_t_tables_host(int(d), float(dof), ptr(lg), ptr(g)))
    return lg, g


def _t_dof_root(q: float, lo: float = 0.5, hi: float = 1e4) -> float:
    """The root of ln(nu / 2) - psi(nu / 2) + 1 + q = 0 by bisection on [lo, hi]; the upper end when there is no sign change.
    -(psi(x) - ln x) comes from ppca_t_tables_host (its g[0] at nu = 2 x)."""
    def f(nu):
        return -_t_tables(0, nu)[1][0] + 1.0 + q
    flo, fhi = f(lo), f(hi)
    if not (flo > 0.0 and fhi < 0.0):  # f falls from +inf to 1 + q: no sign change in the bracket (or q is not a number)
        return hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) > 0.0:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-13 * hi:
            break
    return 0.5 * (lo + hi)


class TPPCAModel:
    """Masked Student-t PPCA: a row is y = mean + (C x + noise) / sqrt(u) with x ~ N(0, I), noise ~ N(0, isotropic_noise^2 I) and a
    latent scale u ~ Gamma(dof / 2, rate dof / 2) per row, so outlying rows get a small weight E[u | y] instead of pulling the mean,
    the subspace and the noise (an extension with no reference counterpart; include/ppca_hip.h).

    Given u a row is a Gaussian row scaled by 1 / sqrt(u): an iteration is one streaming sweep (distances, weights, log-densities, the
    scaled rows, a few column sums) and the EM pass of PPCAModel on the scaled rows.  The step is an ECM step (transform, then mean,
    then noise, each given the ones before it), not the reference's EM step; as dof -> infinity it becomes that ECM step of the
    Gaussian model.  LIMITS: state sizes 1 .. 16; output sizes 1 .. 1024 on a `Dataset` (the streaming sweep's register budget), any
    output size on a `SparseDataset`.

    On a `SparseDataset`: llk / llks / row_weights / mahalanobis / infer / predict / iterate* and TPPCATrainer.train
    run on the entries alone, and the scaled rows are a values view of the dataset.  `row_compressed=True` (keyword-only) declares a
    model meant for such data and lifts the constructor's limit on the output size; `init` on a SparseDataset sets it, and every
    model derived from a flagged one carries it.  Not there: score_heldout and TPPCATrainer.select_state_size (TypeError).
    """

    MAX_STATE_SIZE, MAX_OUTPUT_SIZE = 16, 1024

    def __init__(self, isotropic_noise: float, transform, mean, dof: float, *, ctx=None, _estimated_dof: bool = False,
                 row_compressed: bool = False):
        base = PPCAModel(isotropic_noise, transform, mean, ctx=ctx)  # (the checks of transform and mean are PPCAModel's)
        dof = float(dof)
        if not (np.isfinite(dof) and dof > 0.0):
            raise ValueError("dof must be a positive finite number")
        if not (np.isfinite(base._sigma) and base._sigma > 0.0):
            raise ValueError("isotropic_noise must be a positive finite number")
        d, k = base.output_size, base.state_size
        if k < 1 or k > self.MAX_STATE_SIZE or d < 1 or (d > self.MAX_OUTPUT_SIZE and not row_compressed):
            raise ValueError(f"the Student-t sweep covers state sizes 1 .. {self.MAX_STATE_SIZE} and output sizes 1 .. "
                             f"{self.MAX_OUTPUT_SIZE} (got k={k}, d={d})")
        self._base, self._dof, self._ctx, self._estimated = base, dof, ctx, bool(_estimated_dof)
        self._row_compressed = bool(row_compressed)

    # -- getters ----------------------------------------------------------------
    @property
    def isotropic_noise(self) -> float:
        return self._base._sigma

    @property
    def transform(self) -> np.ndarray:
        return self._base._c.copy()

    @property
    def mean(self) -> np.ndarray:
        return self._base._mean.copy()

    @property
    def dof(self) -> float:
        return self._dof

    @property
    def row_compressed(self) -> bool:
        """Whether the model was declared for row-compressed data (no limit on the output size)."""
        return self._row_compressed

    @property
    def output_size(self) -> int:
        return self._base.output_size

    @property
    def state_size(self) -> int:
        return self._base.state_size

    @property
    def n_parameters(self) -> int:
        """The Gaussian count, plus one once the degrees of freedom have been estimated (iterate(..., estimate_dof=True))."""
        return self._base.n_parameters + (1 if self._estimated else 0)

    def __repr__(self) -> str:
        return (f"TPPCAModel(isotropic_noise={self._base._sigma}, transform=array({self._base._c}), mean=array({self._base._mean}), "
                f"dof={self._dof})")

    # -- construction -------------------------------------------------------------
    @staticmethod
    def init(state_size: int, dataset: Dataset, seed: Optional[int] = None, method: str = "random", dof: float = 4.0) -> "TPPCAModel":
        """The start of PPCAModel.init (same seed, same draw; method="pca": its spectral start) with `dof` degrees of freedom.  On a
        SparseDataset the model is flagged row_compressed (and method="pca" raises PPCAModel.init's ValueError)."""
        if state_size < 1:
            raise ValueError("state_size must be >= 1")
        return TPPCAModel.from_ppca(PPCAModel.init(state_size, dataset, seed=seed, method=method), dof,
                                    row_compressed=isinstance(dataset, SparseDataset))

    @staticmethod
    def from_ppca(model: PPCAModel, dof: float, row_compressed: bool = False) -> "TPPCAModel":
        """The t model with the Gaussian model's sigma, C and mean."""
        return TPPCAModel(model._sigma, model._c, model._mean, dof, ctx=model._ctx, row_compressed=row_compressed)

    def gaussian(self) -> PPCAModel:
        """PPCAModel with the same sigma, C and mean (the limit dof -> infinity)."""
        return self._base

    def to_canonical(self) -> "TPPCAModel":
        """The rotation of PPCAModel.to_canonical on C; sigma, mean and dof are untouched."""
        b = self._base.to_canonical()
        return TPPCAModel(b._sigma, b._c, b._mean, self._dof, ctx=self._ctx, _estimated_dof=self._estimated,
                          row_compressed=self._row_compressed)

    def sample(self, dataset_size: int, mask_prob: float, seed: Optional[int] = None, *, ctx=None) -> Dataset:
        """Host-side numpy (like posterior_sampler(), not a GPU path): Gaussian rows C x + noise, divided by sqrt(u) with
        u ~ Gamma(dof / 2, rate dof / 2), the mean added, then masked independently with probability mask_prob."""
        if not (0.0 <= mask_prob <= 1.0):
            raise ValueError("invalid mask probability")
        rng = np.random.default_rng(seed)
        n, d, k = int(dataset_size), self.output_size, self.state_size
        rows = rng.standard_normal((n, k)) @ self._base._c.T + self._base._sigma * rng.standard_normal((n, d))
        u = rng.gamma(0.5 * self._dof, 2.0 / self._dof, size=n)
        x = self._base._mean + rows / np.sqrt(u)[:, None]
        x[rng.random((n, d)) < mask_prob] = np.nan
        return Dataset(x, ctx=ctx or self._ctx)

    # -- passes ---------------------------------------------------------------------
    def _estep(self, dataset: Dataset, *, scaled: bool = False, col_sums: bool = False, u: bool = False, maha: bool = False,
               llks: bool = False, scalars: bool = False):
        """ppca_t_estep: (scaled rows as a Dataset, column sums V | A | T | sq, u, delta, llks, scalars), None where not asked for.
        On a SparseDataset ppca_t_sparse_estep: the scaled rows are a values view of it, a SparseDataset whose values
        come to the host if csr() / to_dense() asks for them, not before (as SparseDataset._scale_columns's)."""
        if dataset._d != self.output_size:
            raise ValueError(f"dataset has {dataset._d} dimensions but the model has output size {self.output_size}")
        ctx, n, d, k = dataset._ctx, len(dataset), self.output_size, self.state_size
        h = C.c_void_p()
        cs = np.empty((k + 3) * d) if col_sums else None
        uu, mm, ll = (np.empty(n) if f else None for f in (u, maha, llks))
        sc = np.empty(4) if scalars else None
        if isinstance(dataset, SparseDataset):
            check(lib().ppca_t_sparse_estep(ctx.handle, dataset._sh, self._base._device(ctx).h, self._dof, C.byref(h) if scaled else None,
                                            ptr(cs), ptr(uu), ptr(mm), ptr(ll), ptr(sc)))
            view = None
            if scaled:
                view = SparseDataset.__new__(SparseDataset)
                view.__dict__.update(dataset.__dict__)
                view.__dict__.pop("holdout_counts", None)
                view._vals, view._handle = None, h
            return view, cs, uu, mm, ll, sc
        check(lib().ppca_t_estep(ctx.handle, dataset._h, self._base._device(ctx).h, self._dof, C.byref(h) if scaled else None, ptr(cs),
                                 ptr(uu), ptr(mm), ptr(ll), ptr(sc)))
        return (Dataset._wrap(h, ctx) if scaled else None), cs, uu, mm, ll, sc

    def llks(self, dataset: Dataset) -> np.ndarray:
        """Per-sample t log-density of the observed entries (0 for a row without any)."""
        return self._estep(dataset, llks=True)[4]

    def llk(self, dataset: Dataset) -> float:
        """Weighted t log-likelihood."""
        return float(self._estep(dataset, scalars=True)[5][1])

    def row_weights(self, dataset: Dataset) -> np.ndarray:
        """The rows' weights E[u | y] = (dof + m) / (dof + delta): a per-row anomaly score from one pass -- small means outlying; at
        most (dof + m) / dof; 1 for a row without an observed entry."""
        return self._estep(dataset, u=True)[2]

    def mahalanobis(self, dataset: Dataset):
        """(delta, m): the rows' squared Mahalanobis distances (x - mean)_O^T (C_O C_O^T + sigma^2 I)^-1 (x - mean)_O and their
        numbers of observed entries (a second streaming pass counts them; on a SparseDataset they are the rows' lengths)."""
        delta = self._estep(dataset, maha=True)[3]
        if isinstance(dataset, SparseDataset):
            return delta, np.diff(dataset._indptr).astype(np.int64)
        m = dataset._scale_columns(np.ones(self.output_size), l=np.ones(self.output_size), out=False, row_sums=True)[2]
        return delta, np.rint(m).astype(np.int64)

    def infer(self, dataset: Dataset) -> "InferredMasked":
        """The posterior of gaussian(): the posterior mean of the state does not depend on dof; covariances() are the u = 1
        covariances (given the row's scale u they are these divided by u)."""
        return self._base.infer(dataset)

    def predict(self, sparse: "SparseDataset", query):
        """gaussian().predict: (mean, var) of a new reading at the query positions of row-compressed data.  As with `infer`, the mean
        mean_j + c_j . z does not depend on dof, and the variance is the u = 1 variance (given the row's scale u it is this divided
        by u)."""
        return self._base.predict(sparse, query)

    def smooth(self, dataset: Dataset) -> Dataset:
        """C z + mean for every dimension (gaussian().smooth)."""
        return self._base.smooth(dataset)

    def extrapolate(self, dataset: Dataset) -> Dataset:
        """Observed values kept, masked ones replaced by C z + mean (gaussian().extrapolate)."""
        return self._base.extrapolate(dataset)

    def score_heldout(self, train: Dataset, held: Dataset) -> "HeldOutScore":
        """PPCAModel.heldout_score under the t model (module function `heldout_score` calls it for this family): given the m entries of a row in `train`, a held entry is a univariate t with
        dof + m degrees of freedom around mean_j + c_j . z, of scale (sigma^2 + c_j^T Sigma c_j) (dof + delta) / (dof + m) -- an
        outlying row (large delta) widens its own predictive.  z2 takes the variance scale (dof + m) / (dof + m - 2); where
        dof + m <= 2 there is none and the entry adds 0 to it.  One pass on the GPU; nothing of size N x d is allocated."""
        _t_no_sparse_score("TPPCAModel.score_heldout", train, held)
        if train._d != self.output_size:
            raise ValueError(f"dataset has {train._d} dimensions but the model has output size {self.output_size}")
        ctx = train._ctx
        return _heldout_call(train, held, lambda t, c, r: lib().ppca_t_heldout_score(ctx.handle, train._h, held._h,
                                                                                     self._base._device(ctx).h, self._dof, t, c, r))

    def _iterate(self, dataset: Dataset, estimate_dof: bool, want_llk: bool):
        if len(dataset) == 0:
            raise ValueError("dataset is empty")
        d, k = self.output_size, self.state_size
        if dataset._d != d:
            raise ValueError(f"dataset has {dataset._d} dimensions but the model has output size {d}")
        ctx = dataset._ctx
        s_out, c_out, m_out = C.c_double(0.0), np.empty((d, k)), np.empty(d)
        llk, q = C.c_double(0.0), C.c_double(0.0)
        sparse = isinstance(dataset, SparseDataset)
        fn, h = (lib().ppca_t_sparse_em_step, dataset._sh) if sparse else (lib().ppca_t_em_step, dataset._h)
        check(fn(ctx.handle, h, d, k, self._base._sigma, ptr(self._base._c), ptr(self._base._mean), self._dof,
                 C.byref(s_out), ptr(c_out), ptr(m_out), C.byref(llk) if want_llk else None, C.byref(q) if estimate_dof else None))
        dof = _t_dof_root(q.value) if estimate_dof else self._dof
        new = TPPCAModel(s_out.value, c_out, m_out, dof, ctx=self._ctx, _estimated_dof=self._estimated or estimate_dof,
                         row_compressed=self._row_compressed or sparse)
        return new, (llk.value if want_llk else None)

    def iterate(self, dataset: Dataset, estimate_dof: bool = False) -> "TPPCAModel":
        """One ECM iteration (transform, then mean, then noise, each given the ones before it; with estimate_dof then dof, the root
        of ln(nu / 2) - psi(nu / 2) + 1 + q = 0 on [0.5, 1e4]): the t log-likelihood cannot decrease.  `dataset` may be a
        SparseDataset (ppca_t_sparse_em_step)."""
        return self._iterate(dataset, estimate_dof, False)[0]

    def iterate_with_llk(self, dataset: Dataset, estimate_dof: bool = False):
        """(next model, t log-likelihood of THIS model) from the same pass."""
        return self._iterate(dataset, estimate_dof, True)

    # -- serialisation (own npz container) ----------------------------------------------
    def dump(self) -> bytes:
        return _npz_dump("ppca_rs_amd.TPPCAModel", isotropic_noise=self._base._sigma, transform=self._base._c, mean=self._base._mean,
                         dof=self._dof, estimated_dof=self._estimated,
                         # (an unflagged model dumps the container it always dumped: absent reads as off)
                         **({"row_compressed": True} if self._row_compressed else {}))

    @staticmethod
    def load(data: bytes) -> "TPPCAModel":
        return _npz_load(data, "ppca_rs_amd.TPPCAModel", "a TPPCAModel",
                         lambda z: TPPCAModel(float(z["isotropic_noise"]), z["transform"], z["mean"], float(z["dof"]),
                                              _estimated_dof=bool(z["estimated_dof"]),
                                              # (a dump from before the flag existed has no such entry: off)
                                              row_compressed=bool(z["row_compressed"]) if "row_compressed" in z.files else False))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        self.__dict__.update(TPPCAModel.load(state).__dict__)

    def __getnewargs__(self):
        return (self.isotropic_noise, self.transform, self.mean, self.dof)


def _t_no_sparse_score(what: str, *datasets) -> None:
    """The t predictive is not built on row-compressed data: raised before anything touches a device."""
    if any(isinstance(ds, SparseDataset) for ds in datasets):
        raise TypeError(f"{what} is not available on a SparseDataset: held-out scoring under the t model is not built on row-compressed "
                        "data (DESIGN.md section 7); PPCAModel.heldout_score scores the two parts of SparseDataset.holdout under "
                        "gaussian()")


@dataclass
class TPPCATrainer:
    """EM driver of TPPCAModel: the loop and metrics of FATrainer.  `dataset` may be a SparseDataset (train; init="pca" raises
    PPCAModel.init's ValueError)."""

    dataset: Dataset

    def train(self, *, state_size: int, dof: float = 4.0, estimate_dof: bool = False, n_iters: int = 10,
              start: Optional[TPPCAModel] = None, metric: Literal["aic", "bic", "llk"] = "aic", quiet: bool = False,
              seed: Optional[int] = None, init: str = "random") -> TPPCAModel:
        """init: the method of PPCAModel.init ("random" or "pca"), used only when `start` is None.  estimate_dof: update the degrees
        of freedom in every iteration (they start at `dof`, or at start.dof)."""
        ds = self.dataset
        model = start or TPPCAModel.init(state_size, ds, seed=seed, method=init, dof=dof)
        return _train_loop(model, n_iters, quiet, metric, "t-PPCA", len(ds), lambda m: m.iterate_with_llk(ds, estimate_dof),
                           lambda m: m.iterate(ds, estimate_dof),
                           # (a dof about to be estimated for the first time counts as a parameter already)
                           n_parameters=lambda m: m.n_parameters + (1 if estimate_dof and not m._estimated else 0))

    def select_state_size(self, state_sizes, *, fraction: float = 0.1, seed: Optional[int] = None, n_iters: int = 10,
                          init: str = "random", dof: float = 4.0, estimate_dof: bool = False, folds: int = 1):
        """PPCATrainer.select_state_size with TPPCAModel fits at `dof` degrees of freedom (estimated from there with estimate_dof),
        scored by the t predictive: [(state_size, HeldOutScore, TPPCAModel)].  Not on a SparseDataset (TypeError)."""
        _t_no_sparse_score("TPPCATrainer.select_state_size", self.dataset)
        return _select_state_size(self.dataset, state_sizes, fraction, seed, lambda tr, k: TPPCATrainer(tr).train(
            state_size=k, dof=dof, estimate_dof=estimate_dof, n_iters=n_iters, quiet=True, seed=seed, init=init), folds)


# --------------------------------------------------------------------------- PPCA with a known precision per entry
class HPPCAModel:
    """Masked PPCA with a KNOWN precision per entry (weighted / heteroscedastic PCA): x_ij = mean_j + c_j . z_i + eps_ij with
    z_i ~ N(0, I) and eps_ij ~ N(0, isotropic_noise^2 / p_ij), p_ij > 0 given with the data -- an entry that is a mean over n_ij
    readings, or comes with an error bar, enters at its own noise level instead of at full weight or not at all (an extension with no
    reference counterpart; include/ppca_hip.h).  With every precision 1 this is PPCAModel.

    Every pass takes (dataset, precisions): `precisions` is a Dataset, or an array, of the dataset's shape.  An entry is observed iff
    its value is finite and its precision is finite and > 0; a precision of NaN or 0 masks the entry whatever its value; a negative or
    +inf precision raises PPCAError (PPCA_ERR_INVALID).  An iteration is an ECM step (transform, then mean, then noise, each given the
    ones before it, all from one E-step), not the reference's EM step.  LIMITS: state sizes 1 .. 16; output sizes 1 .. 1024 on a
    `Dataset` (the dense sweep's register budget), any output size on a `SparseDataset`.

    On a `SparseDataset`: llk / llks / infer / predict / iterate* and HPPCATrainer.train take (sparse, precisions),
    `precisions` a 1-D array of length nnz aligned with `sparse.csr()[2]`, or a SparseDataset of the identical pattern
    (`sparse.with_values(p)`, or a part of its split).  THE RULE DIFFERS FROM THE DENSE ONE: an entry is observed iff it is stored,
    and every stored entry needs a precision that is finite and > 0 -- there is no masking precision on this data (0, NaN, a negative
    or an infinite one raise ValueError before a device is touched); an entry that should not count is not stored.
    `row_compressed=True` (keyword-only) declares a model meant for such data and lifts the constructor's limit on the output size;
    `init` on a SparseDataset sets it, and every model derived from a flagged one carries it.  Not there: smooth / extrapolate (use
    predict), score_heldout and HPPCATrainer.select_state_size (TypeError).
    """

    MAX_STATE_SIZE, MAX_OUTPUT_SIZE = 16, 1024

    def __init__(self, isotropic_noise: float, transform, mean, *, ctx=None, row_compressed: bool = False):
        base = PPCAModel(isotropic_noise, transform, mean, ctx=ctx)  # (the checks of transform and mean are PPCAModel's)
        if not (np.isfinite(base._sigma) and base._sigma > 0.0):
            raise ValueError("isotropic_noise must be a positive finite number")
        d, k = base.output_size, base.state_size
        if k < 1 or k > self.MAX_STATE_SIZE or d < 1 or (d > self.MAX_OUTPUT_SIZE and not row_compressed):
            raise ValueError(f"the per-entry-precision sweep covers state sizes 1 .. {self.MAX_STATE_SIZE} and output sizes 1 .. "
                             f"{self.MAX_OUTPUT_SIZE} (got k={k}, d={d})")
        self._base, self._ctx = base, ctx
        self._row_compressed = bool(row_compressed)

    # -- getters ----------------------------------------------------------------
    @property
    def isotropic_noise(self) -> float:
        return self._base._sigma

    @property
    def transform(self) -> np.ndarray:
        return self._base._c.copy()

    @property
    def mean(self) -> np.ndarray:
        return self._base._mean.copy()

    @property
    def output_size(self) -> int:
        return self._base.output_size

    @property
    def state_size(self) -> int:
        return self._base.state_size

    @property
    def n_parameters(self) -> int:
        return self._base.n_parameters

    @property
    def row_compressed(self) -> bool:
        """Whether the model was declared for row-compressed data (no limit on the output size)."""
        return self._row_compressed

    def __repr__(self) -> str:
        return f"HPPCAModel(isotropic_noise={self._base._sigma}, transform=array({self._base._c}), mean=array({self._base._mean}))"

    # -- construction -------------------------------------------------------------
    @staticmethod
    def init(state_size: int, dataset: Dataset, seed: Optional[int] = None, method: str = "random") -> "HPPCAModel":
        """The start of PPCAModel.init (same seed, same draw; method="pca": its spectral start through PPCAModel.from_moments, which
        ignores the precisions).  On a SparseDataset the model is flagged row_compressed (and method="pca" raises PPCAModel.init's
        ValueError)."""
        if state_size < 1:
            raise ValueError("state_size must be >= 1")
        return HPPCAModel.from_ppca(PPCAModel.init(state_size, dataset, seed=seed, method=method),
                                    row_compressed=isinstance(dataset, SparseDataset))

    @staticmethod
    def from_ppca(model: PPCAModel, row_compressed: bool = False) -> "HPPCAModel":
        return HPPCAModel(model._sigma, model._c, model._mean, ctx=model._ctx, row_compressed=row_compressed)

    def gaussian(self) -> PPCAModel:
        """PPCAModel with the same sigma, C and mean (every precision 1)."""
        return self._base

    def to_canonical(self) -> "HPPCAModel":
        """The rotation of PPCAModel.to_canonical on C; sigma and mean are untouched."""
        b = self._base.to_canonical()
        return HPPCAModel(b._sigma, b._c, b._mean, ctx=self._ctx, row_compressed=self._row_compressed)

    def sample(self, precisions, seed: Optional[int] = None, *, ctx=None) -> Dataset:
        """Host-side numpy (like TPPCAModel.sample): one row per row of `precisions` (an array or a Dataset, N x output_size),
        mean + C z + isotropic_noise eps / sqrt(p) -- every entry at the noise level its precision gives; NaN where the precision
        is NaN or 0."""
        p = precisions.numpy() if isinstance(precisions, Dataset) else np.asarray(precisions, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.output_size:
            raise ValueError(f"precisions must be (N, {self.output_size}); got {p.shape}")
        if (p < 0).any() or np.isposinf(p).any():
            raise ValueError("a precision is negative or +inf")
        rng = np.random.default_rng(seed)
        n, d, k = p.shape[0], self.output_size, self.state_size
        on = np.isfinite(p) & (p > 0)
        rows = rng.standard_normal((n, k)) @ self._base._c.T
        eps = rng.standard_normal((n, d))
        x = self._base._mean + rows + self._base._sigma * eps / np.sqrt(np.where(on, p, 1.0))
        x[~on] = np.nan
        return Dataset(x, ctx=ctx or self._ctx)

    # -- passes ---------------------------------------------------------------------
    def _pair(self, dataset: Dataset, precisions) -> Dataset:
        """`precisions` as a Dataset on the dataset's context, shapes checked."""
        n, d = len(dataset), dataset._d
        if d != self.output_size:
            raise ValueError(f"dataset has {d} dimensions but the model has output size {self.output_size}")
        if not isinstance(precisions, Dataset):
            p = np.ascontiguousarray(precisions, dtype=np.float64)
            if p.shape != (n, d):
                raise ValueError(f"precisions have shape {p.shape} but the dataset is {n} x {d}")
            precisions = Dataset(p, ctx=dataset._ctx)
        return precisions

    def _sparse_pair(self, sparse: "SparseDataset", precisions) -> "_SparsePrecisions":
        """`precisions` as a device view of `sparse` (ppca_h_sparse_precisions): a 1-D array of length nnz aligned
        with sparse.csr()[2], a SparseDataset of the identical pattern, or a view built before (HPPCATrainer builds it once).  Every
        check comes before a device is touched."""
        if sparse._d != self.output_size:
            raise ValueError(f"dataset has {sparse._d} dimensions but the model has output size {self.output_size}")
        if len(sparse) == 0:
            raise ValueError("dataset is empty")
        if isinstance(precisions, _SparsePrecisions):
            if not precisions._matches(sparse):
                raise ValueError("the precisions were prepared for a dataset of another pattern")
            return precisions
        return _SparsePrecisions(sparse, precisions)

    def _estep(self, dataset: Dataset, precisions, *, llks: bool = False, states: bool = False, covs: bool = False, stats: bool = False,
               scalars: bool = False):
        """ppca_h_estep: (llks, states, covs, statistics, scalars), None where not asked for.  On a SparseDataset
        ppca_h_sparse_estep."""
        sparse = isinstance(dataset, SparseDataset)
        prec = self._sparse_pair(dataset, precisions) if sparse else self._pair(dataset, precisions)
        ctx, n, d, k = dataset._ctx, len(dataset), self.output_size, self.state_size
        ll = np.empty(n) if llks else None
        st = np.empty((n, k)) if states else None
        cv = np.empty((n, k, k)) if covs else None
        ss = np.empty(int(lib().ppca_h_stats_len(d, k))) if stats else None
        sc = np.empty(4) if scalars else None
        if sparse:
            check(lib().ppca_h_sparse_estep(self._base._device(ctx).h, ctx.handle, dataset._sh, prec._handle, ptr(ll), ptr(st), ptr(cv),
                                            ptr(ss), ptr(sc)))
        else:
            check(lib().ppca_h_estep(ctx.handle, dataset._h, prec._h, self._base._device(ctx).h, ptr(ll), ptr(st), ptr(cv), ptr(ss), ptr(sc)))
        return ll, st, cv, ss, sc

    def predict(self, sparse: "SparseDataset", precisions, query):
        """PPCAModel.predict under this model's posterior: (mean, var) at the query positions (a SparseDataset of the same rows, or an
        (indptr, indices) pair), given the row's stored entries at their precisions.  mean = mean_j + c_j . z;
        var = c_j^T Sigma c_j + sigma^2 is the predictive variance of a reading at UNIT precision -- one taken at precision q has
        var + sigma^2 (1 / q - 1).  A row without an entry gives the prior predictive (mean_j, |c_j|^2 + sigma^2)."""
        if not isinstance(sparse, SparseDataset):
            raise TypeError("predict takes a SparseDataset; on a Dataset use smooth / extrapolate")
        prec = self._sparse_pair(sparse, precisions)
        ip, ix = _query_pattern(sparse, query)
        ctx = sparse._ctx
        mean, var = np.empty(ix.size), np.empty(ix.size)
        check(lib().ppca_h_sparse_predict(self._base._device(ctx).h, ctx.handle, sparse._sh, prec._handle, ptr(ip), ptr(ix), ptr(mean),
                                          ptr(var)))
        return mean, var

    def llks(self, dataset: Dataset, precisions) -> np.ndarray:
        """Per-sample log-density of the observed entries (0 for a row without any)."""
        return self._estep(dataset, precisions, llks=True)[0]

    def llk(self, dataset: Dataset, precisions) -> float:
        """Weighted log-likelihood."""
        return float(self._estep(dataset, precisions, scalars=True)[4][1])

    def infer(self, dataset: Dataset, precisions) -> InferredFA:
        """Posterior means z_i = M_i^-1 b_i and covariances sigma^2 M_i^-1 of the latent states."""
        _, st, cv, _, _ = self._estep(dataset, precisions, states=True, covs=True)
        return InferredFA(st, cv)

    def _recon(self, dataset: Dataset, precisions, mode: int) -> Dataset:
        if isinstance(dataset, SparseDataset):
            raise TypeError("smooth / extrapolate are not available on a SparseDataset (their output is N x d): "
                            "HPPCAModel.predict(sparse, precisions, query) gives the reconstruction at the positions asked for")
        prec = self._pair(dataset, precisions)
        ctx = dataset._ctx
        h = C.c_void_p()
        check(lib().ppca_h_reconstruct(ctx.handle, dataset._h, prec._h, self._base._device(ctx).h, mode, C.byref(h)))
        return Dataset._wrap(h, ctx)

    def smooth(self, dataset: Dataset, precisions) -> Dataset:
        """C z + mean for every dimension."""
        return self._recon(dataset, precisions, 0)

    def extrapolate(self, dataset: Dataset, precisions) -> Dataset:
        """Observed values kept (observed: finite value, finite precision > 0), the others replaced by C z + mean."""
        return self._recon(dataset, precisions, 1)

    def score_heldout(self, train: Dataset, held: Dataset, precisions, held_precisions=None) -> "HeldOutScore":
        """PPCAModel.heldout_score under known precisions (module function `heldout_score` calls it for this family): the posterior of a row from its entries in `train` under `precisions`,
        then every entry of `held` that is observed under `held_precisions` (default: `precisions` -- after a split of the values the
        precisions of both parts are the same array) scored at its own noise level, v = sigma^2 / q + c_j^T Sigma c_j.  A negative or
        +inf precision raises PPCAError.  One pass on the GPU; nothing of size N x d is allocated.  Not on SparseDatasets (TypeError)."""
        _h_no_sparse_score("HPPCAModel.score_heldout", train, held)
        if len(train) != len(held) or train._d != held._d:
            raise ValueError("the train part and the held part differ in shape")
        prec = self._pair(train, precisions)
        hprec = prec if held_precisions is None else self._pair(held, held_precisions)
        ctx = train._ctx
        return _heldout_call(train, held, lambda t, c, r: lib().ppca_h_heldout_score(ctx.handle, train._h, prec._h, held._h, hprec._h,
                                                                                     self._base._device(ctx).h, t, c, r))

    def _iterate(self, dataset: Dataset, precisions, want_llk: bool):
        if len(dataset) == 0:
            raise ValueError("dataset is empty")
        sparse = isinstance(dataset, SparseDataset)
        prec = self._sparse_pair(dataset, precisions) if sparse else self._pair(dataset, precisions)
        ctx, d, k = dataset._ctx, self.output_size, self.state_size
        s_out, c_out, m_out, llk = C.c_double(0.0), np.empty((d, k)), np.empty(d), C.c_double(0.0)
        if sparse:
            check(lib().ppca_h_sparse_em_step(d, k, self._base._sigma, ptr(self._base._c), ptr(self._base._mean), ctx.handle, dataset._sh,
                                              prec._handle, C.byref(s_out), ptr(c_out), ptr(m_out), C.byref(llk) if want_llk else None))
        else:
            check(lib().ppca_h_em_step(ctx.handle, dataset._h, prec._h, d, k, self._base._sigma, ptr(self._base._c), ptr(self._base._mean),
                                       C.byref(s_out), ptr(c_out), ptr(m_out), C.byref(llk) if want_llk else None))
        return (HPPCAModel(s_out.value, c_out, m_out, ctx=self._ctx, row_compressed=self._row_compressed or sparse),
                (llk.value if want_llk else None))

    def iterate(self, dataset: Dataset, precisions) -> "HPPCAModel":
        """One ECM iteration: the log-likelihood cannot decrease.  `dataset` may be a SparseDataset (ppca_h_sparse_em_step, DESIGN.md
        4.30)."""
        return self._iterate(dataset, precisions, False)[0]

    def iterate_with_llk(self, dataset: Dataset, precisions):
        """(next model, log-likelihood of THIS model) from the same pass."""
        return self._iterate(dataset, precisions, True)

    # -- serialisation (own npz container) ----------------------------------------------
    def dump(self) -> bytes:
        return _npz_dump("ppca_rs_amd.HPPCAModel", isotropic_noise=self._base._sigma, transform=self._base._c, mean=self._base._mean,
                         # (an unflagged model dumps the container it always dumped: absent reads as off)
                         **({"row_compressed": True} if self._row_compressed else {}))

    @staticmethod
    def load(data: bytes) -> "HPPCAModel":
        return _npz_load(data, "ppca_rs_amd.HPPCAModel", "a HPPCAModel",
                         lambda z: HPPCAModel(float(z["isotropic_noise"]), z["transform"], z["mean"],
                                              row_compressed=bool(z["row_compressed"]) if "row_compressed" in z.files else False))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        self.__dict__.update(HPPCAModel.load(state).__dict__)

    def __getnewargs__(self):
        return (self.isotropic_noise, self.transform, self.mean)


class _SparsePrecisions:
    """The precisions of a SparseDataset's entries on the device: a values view of the dataset (ppca_h_sparse_precisions, DESIGN.md
    4.30) that shares its pattern, row lists, inverted index and work items.  Everything is checked on the host first -- the length
    or the pattern, then every precision finite and > 0 -- and only then does the dataset go to the device."""

    def __init__(self, sparse: SparseDataset, precisions):
        if isinstance(precisions, SparseDataset):
            if (precisions._d != sparse._d or not np.array_equal(precisions._indptr, sparse._indptr)
                    or not np.array_equal(precisions._indices, sparse._indices)):
                raise ValueError("the precisions and the dataset differ in pattern: a precision belongs to every stored entry and to "
                                 "no other position")
            p = precisions._values
        else:
            p = np.ascontiguousarray(np.asarray(precisions), dtype=np.float64)
            if p.ndim != 1 or p.shape[0] != sparse.nnz:
                raise ValueError(f"precisions have shape {p.shape} but the dataset stores {sparse.nnz} entries: one precision per stored "
                                 "entry, aligned with csr()[2]")
        if not (np.isfinite(p) & (p > 0.0)).all():
            raise ValueError("every stored entry needs a precision that is finite and > 0 (on row-compressed data there is no masking "
                             "precision: an entry that should not count is not stored)")
        self._indptr, self._indices, self._d = sparse._indptr, sparse._indices, sparse._d
        self._tiling = (sparse._block_rows, sparse._segment)
        self._handle = None
        h = C.c_void_p()
        check(lib().ppca_h_sparse_precisions(ptr(p), sparse._ctx.handle, sparse._sh, C.byref(h)))
        self._of, self._handle = sparse._sh, h  # (the library holds the pattern alive; _of names it)

    def _matches(self, sparse: SparseDataset) -> bool:
        """Whether this view was made on the device copy of `sparse` (or of a with_weights sibling made after the upload)."""
        return sparse._handle is not None and (sparse._handle is self._of or (
            sparse._indptr is self._indptr and sparse._indices is self._indices and (sparse._block_rows, sparse._segment) == self._tiling))

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                lib().ppca_sparse_free(self._handle)
                self._handle = None
        except Exception:
            pass


def _h_no_sparse_score(what: str, *datasets) -> None:
    """Held-out scoring under known precisions is not built on row-compressed data: raised before anything touches a device."""
    if any(isinstance(ds, SparseDataset) for ds in datasets):
        raise TypeError(f"{what} is not available on a SparseDataset: held-out scoring under known precisions is not built on "
                        "row-compressed data (DESIGN.md section 7); HPPCAModel.llk / llks / infer / predict / iterate* and "
                        "HPPCATrainer.train are, and PPCAModel.heldout_score scores the two parts of SparseDataset.holdout under "
                        "gaussian()")


@dataclass
class HPPCATrainer:
    """EM driver of HPPCAModel.  train returns (model, metrics): the canonical model after n_iters iterations and one TrainMetrics per
    iteration, of the model that ENTERED it (the log-likelihood is a by-product of the iteration's sweep).  `dataset` may be a
    SparseDataset with `precisions` one value per stored entry (train; init="pca" raises PPCAModel.init's ValueError)."""

    dataset: Dataset
    precisions: object

    def train(self, *, state_size: int, n_iters: int = 10, start: Optional[HPPCAModel] = None, init: str = "random",
              seed: Optional[int] = None, quiet: bool = True, metric: Literal["aic", "bic", "llk"] = "aic"):
        ds = self.dataset
        model = start or HPPCAModel.init(state_size, ds, seed=seed, method=init)
        # (uploaded once; on a SparseDataset the device view is built once)
        prec = model._sparse_pair(ds, self.precisions) if isinstance(ds, SparseDataset) else model._pair(ds, self.precisions)
        metrics: List[TrainMetrics] = []
        for idx in range(n_iters):
            new_model, llk = model.iterate_with_llk(ds, prec)
            metrics.append(_metrics(llk, model.n_parameters, len(ds)))
            if not quiet:
                print(f"Masked H-PPCA iteration {idx + 1}: {metric}={getattr(metrics[-1], metric)}")
            model = new_model
        return model.to_canonical(), metrics

    def select_state_size(self, state_sizes, *, fraction: float = 0.1, seed: Optional[int] = None, n_iters: int = 10,
                          init: str = "random", folds: int = 1):
        """PPCATrainer.select_state_size with HPPCAModel fits under this trainer's precisions, which also are the held entries'
        (the split follows the values): [(state_size, HeldOutScore, HPPCAModel)].  Not on a SparseDataset (TypeError)."""
        _h_no_sparse_score("HPPCATrainer.select_state_size", self.dataset)
        ds = self.dataset
        prec = self.precisions
        if not isinstance(prec, Dataset):
            p = np.ascontiguousarray(prec, dtype=np.float64)
            if p.shape != (len(ds), ds._d):
                raise ValueError(f"precisions have shape {p.shape} but the dataset is {len(ds)} x {ds._d}")
            prec = Dataset(p, ctx=ds._ctx)  # (uploaded once)
        return _select_state_size(ds, state_sizes, fraction, seed, lambda tr, k: HPPCATrainer(tr, prec).train(
            state_size=k, n_iters=n_iters, quiet=True, seed=seed, init=init)[0], folds,
            score=lambda model, train, held: model.score_heldout(train, held, prec))


# --------------------------------------------------------------------------- mixture
def _log_softmax(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    mx = v.max()
    return v - mx - np.log(np.exp(v - mx).sum())


class PPCAMix:
    """Mixture of PPCA models (mix.rs:27-83; src/python_bindings.rs:535-711)."""

    def __init__(self, models: Sequence[PPCAModel], log_weights):
        models = list(models)
        lw = f64(log_weights).ravel()
        if len(models) == 0:
            raise ValueError("need at least one model")  # assert! mix.rs:51
        if len(models) != lw.shape[0]:
            raise ValueError("models and log_weights differ in length")  # mix.rs:52
        sizes = {m.output_size for m in models}
        if len(sizes) != 1:
            raise ValueError(f"Model output sizes are not the same: {[m.output_size for m in models]}")
        self._models = models
        self._lw = _log_softmax(lw)  # mix.rs:69

    @staticmethod
    def init(n_models: int, state_size: int, dataset: Dataset, seed: Optional[int] = None, method: str = "random") -> "PPCAMix":
        """mix.rs:76-83.  method="kmeans" (an extension): `from_kmeans(state_size, dataset, dataset.kmeans(n_models, seed=seed))`."""
        if method == "kmeans":
            if isinstance(dataset, SparseDataset):
                raise ValueError("method='kmeans' is not available on a SparseDataset: k-means takes a dense Dataset")
            return PPCAMix.from_kmeans(state_size, dataset, dataset.kmeans(n_models, seed=seed))
        if method != "random":
            raise ValueError("method must be 'random' or 'kmeans'")
        ss = np.random.SeedSequence(seed)
        seeds = [int(s.generate_state(1)[0]) for s in ss.spawn(n_models)]
        return PPCAMix([PPCAModel.init(state_size, dataset, seed=s) for s in seeds], np.zeros(n_models))

    @staticmethod
    def from_kmeans(state_size: int, dataset: Dataset, km: "KMeans") -> "PPCAMix":
        """The k-means start: component c is `PPCAModel.from_moments` of the rows of cluster c (the dataset under the weights
        w * (km.labels == c): one moment pass per cluster), log_weights = ln(cluster_weights / their sum).  A cluster of weight 0 takes
        the whole dataset's `from_moments` model and the weight of the lightest cluster that has some."""
        if isinstance(dataset, SparseDataset):
            raise ValueError("from_kmeans is not available on a SparseDataset: k-means takes a dense Dataset")
        moms, whole, lw = _kmeans_cluster_moments(dataset, km)
        return PPCAMix([PPCAModel.from_moments(state_size, m if m is not None else whole) for m in moms], lw)

    @property
    def output_size(self) -> int:
        return self._models[0].output_size

    @property
    def state_sizes(self) -> List[int]:
        return [m.state_size for m in self._models]

    @property
    def n_parameters(self) -> int:
        """mix.rs:96-104"""
        return sum(m.n_parameters for m in self._models) + len(self._models) - 1

    @property
    def models(self) -> List[PPCAModel]:
        return list(self._models)

    @property
    def log_weights(self) -> np.ndarray:
        return self._lw.copy()

    @property
    def weights(self) -> np.ndarray:
        return np.exp(self._lw)

    def _handles(self, ctx):
        devs = [m._device(ctx) for m in self._models]
        arr = (C.c_void_p * len(devs))(*[d.h for d in devs])
        return devs, arr

    def _mix_llk(self, dataset: Dataset, total, per_row, log_posteriors):
        """ppca_mix_llk, or ppca_mix_sparse_llk on a SparseDataset; each output nullable."""
        devs, arr = self._handles(dataset._ctx)
        fn, h = (lib().ppca_mix_sparse_llk, dataset._sh) if isinstance(dataset, SparseDataset) else (lib().ppca_mix_llk, dataset._h)
        check(fn(dataset._ctx.handle, h, arr, ptr(self._lw), len(devs), total, per_row, log_posteriors))

    def llk(self, dataset: Dataset) -> float:
        """mix.rs:162-174"""
        tot = C.c_double(0.0)
        self._mix_llk(dataset, C.byref(tot), None, None)
        return tot.value

    def llks(self, dataset: Dataset) -> np.ndarray:
        """mix.rs:152-159"""
        out = np.empty(len(dataset))
        self._mix_llk(dataset, None, ptr(out), None)
        return out

    def infer_cluster(self, dataset: Dataset) -> np.ndarray:
        """Log posteriors (N, n_models) (mix.rs:179-189)."""
        out = np.empty((len(dataset), len(self._models)))
        self._mix_llk(dataset, None, None, ptr(out))
        return out

    def predict(self, sparse: "SparseDataset", query):
        """PPCAModel.predict for the mixture: (mean, var) of a new reading at the query positions of row-compressed data, one value per
        query entry in query order.  With r_c the row's posterior over the components given its entries in `sparse` and (m_c, v_c)
        component c's `predict`: mean = sum_c r_c m_c and var = sum_c r_c v_c + sum_c r_c (m_c - mean)^2 -- the convention of
        InferredMaskedMix.smoothed_covariances_diagonal with sigma^2 included.  No N x d array is formed."""
        if not isinstance(sparse, SparseDataset):
            raise TypeError("predict takes a SparseDataset (on a Dataset: smooth / extrapolate / heldout_score)")
        ip, ix = _query_pattern(sparse, query)
        mean, var = np.empty(ix.size), np.empty(ix.size)
        ctx = sparse._ctx
        devs, arr = self._handles(ctx)
        check(lib().ppca_mix_sparse_predict(ctx.handle, sparse._sh, arr, ptr(self._lw), len(devs), ptr(ip), ptr(ix), ptr(mean), ptr(var)))
        return mean, var

    def recommend(self, sparse: "SparseDataset", n: int, *, kappa: float = 0.0, exclude_observed: bool = True, candidates=None):
        """PPCAModel.recommend for the mixture, in one device pass: for every row of row-compressed data the n columns
        the mixture ranks highest.  The score of column j for row i is mean_ij + kappa sqrt(var_ij) with exactly this mixture's
        `predict`'s two values (the posterior-weighted mean; the weighted variances plus the spread of the components' means), so
        kappa = 0 ranks by the mixture's predictive mean and forms no covariance.  Arguments, checks, order (score descending, equal
        scores by ascending column) and padding (-1 / NaN) are PPCAModel.recommend's; returns (columns int32 (N, n), scores float64
        (N, n)).  Row weights play no part, an empty row ranks under the prior weights, a one-component mixture gives its model's
        `recommend` bit for bit, and no N x d array is formed."""
        n, kappa, cand = _recommend_args(sparse, n, kappa, candidates)
        if self.output_size != sparse._d:
            raise ValueError(f"dataset has {sparse._d} columns but the mixture has output size {self.output_size}")
        if max(self.state_sizes) > 16:  # (the library's own answer, given here so that it comes before the first touch of a device)
            raise _lib.PPCAError(-3, f"state size {max(self.state_sizes)} is not supported on sparse data: the kernels cover k <= 16")
        cols, scores = np.empty((len(sparse), n), dtype=np.int32), np.empty((len(sparse), n))
        if len(sparse) == 0:
            return cols, scores
        ctx = sparse._ctx
        devs, arr = self._handles(ctx)
        cbuf = cand if cand is None or cand.size else np.zeros(1, dtype=np.int32)  # (an empty list is not NULL = every column)
        check(lib().ppca_mix_topn_sparse(ctx.handle, sparse._sh, arr, ptr(self._lw), len(devs), n, kappa, 1 if exclude_observed else 0,
                                         ptr(cbuf), 0 if cand is None else cand.size, ptr(cols), ptr(scores)))
        return cols, scores

    def _iterate(self, dataset: Dataset, prior: Optional[Prior], want_llk: bool):
        if len(dataset) == 0:
            raise ValueError("dataset is empty")
        ctx = dataset._ctx
        devs, arr = self._handles(ctx)
        outs = []
        for m in self._models:
            h = C.c_void_p()
            check(lib().ppca_model_alloc(ctx.handle, m.output_size, m.state_size, C.byref(h)))
            outs.append(_DevModel(h))
        oarr = (C.c_void_p * len(outs))(*[o.h for o in outs])
        lw_out = np.empty(len(outs))
        llk = C.c_double(0.0)
        pref, keep = _prior_ref(prior)
        fn, h = (lib().ppca_mix_sparse_em_step, dataset._sh) if isinstance(dataset, SparseDataset) else (lib().ppca_mix_em_step, dataset._h)
        check(fn(ctx.handle, h, arr, ptr(self._lw), len(devs), pref, oarr, ptr(lw_out), C.byref(llk) if want_llk else None))
        models = [PPCAModel._from_device(o, ctx, m.output_size, m.state_size) for o, m in zip(outs, self._models)]
        new = PPCAMix.__new__(PPCAMix)
        new._models, new._lw = models, lw_out
        return new, (llk.value if want_llk else None)

    def iterate(self, dataset: Dataset) -> "PPCAMix":
        return self._iterate(dataset, None, False)[0]

    def iterate_with_prior(self, dataset: Dataset, prior: Prior) -> "PPCAMix":
        """mix.rs:281-337"""
        return self._iterate(dataset, prior, False)[0]

    def iterate_with_llk(self, dataset: Dataset, prior: Optional[Prior] = None):
        return self._iterate(dataset, prior, True)

    def to_canonical(self) -> "PPCAMix":
        """mix.rs:340-346"""
        new = PPCAMix.__new__(PPCAMix)
        new._models, new._lw = [m.to_canonical() for m in self._models], self._lw.copy()
        return new

    # -- inference outputs (mix.rs:179-265; src/python_bindings.rs:645-672) ---------------------------
    def infer(self, dataset: Dataset) -> "InferredMaskedMix":
        """Posterior over the components and the per-component state posteriors (mix.rs:206-235)."""
        _dense_only(dataset)  # (the accessors of InferredMaskedMix form N x d arrays)
        return InferredMaskedMix(self, self.infer_cluster(dataset), [m.infer(dataset) for m in self._models])

    def _mix_recon(self, dataset: Dataset, mode: int) -> Dataset:
        _dense_only(dataset)
        ctx = dataset._ctx
        devs, arr = self._handles(ctx)
        h = C.c_void_p()
        check(lib().ppca_mix_reconstruct(ctx.handle, dataset._h, arr, ptr(self._lw), len(devs), mode, C.byref(h)))
        return Dataset._wrap(h, ctx)

    def smooth(self, dataset: Dataset) -> Dataset:
        """Posterior-weighted sum of the components' smoothed outputs, on the GPU (mix.rs:238-251, :404-412);
        the result carries no weights, like the reference's."""
        return self._mix_recon(dataset, 0)

    filter_extrapolate = smooth

    def extrapolate(self, dataset: Dataset) -> Dataset:
        """mix.rs:254-265, :414-423"""
        return self._mix_recon(dataset, 1)

    def sample_posterior(self, dataset: Dataset, seed: Optional[int] = None, *, keep_observed: bool = False,
                         row_offset: int = 0) -> Dataset:
        """One draw per row on the GPU: a component from the row's posterior over the components, then that component's
        PPCAModel.sample_posterior draw of the row (same generator, same keep_observed / row_offset meaning).  The result
        carries no weights, like the other mixture outputs.  seed=None draws a fresh seed."""
        if row_offset < 0:
            raise ValueError("row_offset must be >= 0")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        _dense_only(dataset)
        ctx = dataset._ctx
        devs, arr = self._handles(ctx)
        h = C.c_void_p()
        check(lib().ppca_mix_posterior_sample(ctx.handle, dataset._h, arr, ptr(self._lw), len(devs), int(bool(keep_observed)),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), C.byref(h)))
        return Dataset._wrap(h, ctx)

    def heldout_score(self, train: Dataset, held: Dataset) -> "HeldOutScore":
        """PPCAModel.heldout_score for the mixture: per held entry the mixture of the components' predictives, component c weighted
        by its posterior given the row of `train`.  l = logsumexp_c(lp_c + l_c); the error is the mixture mean's, the variance
        sum_c a_c v_c plus the spread of the components' means."""
        _dense_only(train, held)
        ctx = train._ctx
        devs, arr = self._handles(ctx)
        return _heldout_call(train, held, lambda t, c, r: lib().ppca_mix_heldout_score(ctx.handle, train._h, held._h, arr,
                                                                                      ptr(self._lw), len(devs), t, c, r))

    def _loo(self, dataset: Dataset, full: bool, per_sample: bool):
        _dense_only(dataset)
        ctx = dataset._ctx
        devs, arr = self._handles(ctx)
        return _loo_call(dataset, full, per_sample, lambda mh, vh, tot, ps: lib().ppca_mix_loo_predictive(
            ctx.handle, dataset._h, arr, ptr(self._lw), len(devs), mh, vh, tot, ps))

    def loo_predictive(self, dataset: Dataset) -> "LooPredictive":
        """PPCAModel.loo_predictive for the mixture: per entry the mixture of the components' leave-one-out predictives, each
        component weighted by its posterior given the row without that entry (masked entries: by its posterior given the
        row, as `extrapolate` does).  The datasets carry no weights, like the other mixture outputs."""
        return self._loo(dataset, True, True)

    def loo_llks(self, dataset: Dataset) -> np.ndarray:
        """PPCAModel.loo_llks for the mixture (no N x d output is written)."""
        return self._loo(dataset, False, True)._llks

    def loo_llk(self, dataset: Dataset) -> float:
        """sum_i w_i loo_llks[i], the sample weights applied as in `llk`."""
        return self._loo(dataset, False, False)._llk

    def sample(self, dataset_size: int, mask_prob: float, seed: Optional[int] = None) -> Dataset:
        """mix.rs:124-134: a component per sample from the prior weights, then that component's generative
        process (component blocks are generated on the GPU and interleaved by a random permutation)."""
        if not (0.0 <= mask_prob <= 1.0):
            raise ValueError("invalid mask probability")
        rng = np.random.default_rng(seed)
        which = rng.choice(len(self._models), size=dataset_size, p=self.weights / self.weights.sum())
        out = np.empty((dataset_size, self.output_size))
        for c, m in enumerate(self._models):
            idx = np.nonzero(which == c)[0]
            if idx.size:
                out[idx] = m.sample(idx.size, mask_prob, seed=int(rng.integers(0, 2 ** 63 - 1))).numpy()
        return Dataset(out)

    # -- serialisation (own container; bincode layout is a "next" row) ---------------------------------
    def dump(self, format: str = "npz") -> bytes:
        if format == "bincode":
            return _wire.dump_mix([(m._sigma, m._c, m._mean) for m in self._models], self._lw)
        buf = io.BytesIO()
        np.savez(buf, kind="ppca_rs_amd.PPCAMix", log_weights=self._lw, n_models=len(self._models),
                 **{f"sigma_{i}": m._sigma for i, m in enumerate(self._models)},
                 **{f"transform_{i}": m._c for i, m in enumerate(self._models)},
                 **{f"mean_{i}": m._mean for i, m in enumerate(self._models)})
        return buf.getvalue()

    @staticmethod
    def load(data: bytes) -> "PPCAMix":
        try:
            if bytes(data[:2]) != b"PK":
                models, lw = _wire.load_mix(data)
                return PPCAMix([PPCAModel(*m) for m in models], lw)
            z = np.load(io.BytesIO(data), allow_pickle=False)
            nm = int(z["n_models"])
            return PPCAMix([PPCAModel(float(z[f"sigma_{i}"]), z[f"transform_{i}"], z[f"mean_{i}"]) for i in range(nm)],
                           z["log_weights"])
        except Exception as err:
            raise Exception(str(err))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        o = PPCAMix.load(state)
        self.__dict__.update(o.__dict__)

    def __getnewargs__(self):
        return (self.models, self.log_weights)


class InferredMaskedMix:
    """Batch of mixture posteriors (mix.rs:349-515; src/python_bindings.rs:713-885).  The per-sample inference
    ran on the GPU (PPCAMix.infer); these accessors combine the already-inferred host arrays exactly as the
    reference's do, quirks included."""

    def __init__(self, mix: PPCAMix, log_posterior: np.ndarray, inferred: List["InferredMasked"]):
        self._mix, self._lp, self._inf = mix, log_posterior, inferred

    def log_posteriors(self) -> np.ndarray:
        if self._lp.shape[0] == 0:
            return np.zeros((0, 0))
        return self._lp.copy()

    def posteriors(self) -> np.ndarray:
        if self._lp.shape[0] == 0:
            return np.zeros((0, 0))
        return np.exp(self._lp)

    def sub_states(self) -> List["InferredMasked"]:
        return list(self._inf)

    def _state_stack(self) -> np.ndarray:  # (K, N, k)
        return np.stack([i._states for i in self._inf])

    def states(self) -> np.ndarray:
        """mix.rs:374-380 -- as written upstream the components are weighted by the LOG posterior."""
        if self._lp.shape[0] == 0:
            return np.zeros((0, 0))
        return np.einsum("nc,cnk->nk", self._lp, self._state_stack())

    def covariances(self) -> List[np.ndarray]:
        """mix.rs:383-396: sum_c post_c (Sigma_c + (z_c - mean)(z_c - mean)^T), mean = states()."""
        mean, post, zs = self.states(), np.exp(self._lp), self._state_stack()
        out = []
        for i in range(self._lp.shape[0]):
            acc = 0.0
            for c, inf in enumerate(self._inf):
                dv = zs[c, i] - mean[i]
                acc = acc + post[i, c] * (inf._covs[i] + np.outer(dv, dv))
            out.append(acc)
        return out

    def _weighted(self, per_model: List[np.ndarray]) -> np.ndarray:
        return np.einsum("nc,cnj->nj", np.exp(self._lp), np.stack(per_model))

    def smoothed(self, ppca: PPCAMix) -> Dataset:
        """mix.rs:399-407"""
        return Dataset(np.ascontiguousarray(self._weighted([i.smoothed(m).numpy() for i, m in zip(self._inf, ppca._models)])))

    def extrapolated(self, ppca: PPCAMix, dataset: Dataset) -> Dataset:
        """mix.rs:410-418"""
        return Dataset(np.ascontiguousarray(
            self._weighted([i.extrapolated(m, dataset).numpy() for i, m in zip(self._inf, ppca._models)])))

    def _cov_sum(self, means: List[np.ndarray], covs: List[List[np.ndarray]]) -> List[np.ndarray]:
        post = np.exp(self._lp)
        mean = np.einsum("nc,cnj->nj", post, np.stack(means))
        out = []
        for i in range(self._lp.shape[0]):
            acc = 0.0
            for c in range(len(self._inf)):
                dv = means[c][i] - mean[i]
                acc = acc + post[i, c] * (covs[c][i] + np.outer(dv, dv))
            out.append(acc)
        return out

    def smoothed_covariances(self, ppca: PPCAMix) -> List[np.ndarray]:
        """mix.rs:426-440 -- d x d per sample."""
        return self._cov_sum([i.smoothed(m).numpy() for i, m in zip(self._inf, ppca._models)],
                             [i.smoothed_covariances(m) for i, m in zip(self._inf, ppca._models)])

    def smoothed_covariances_diagonal(self, ppca: PPCAMix) -> Dataset:
        """mix.rs:447-461"""
        sm = [i.smoothed(m).numpy() for i, m in zip(self._inf, ppca._models)]
        mean = self._weighted(sm)
        dg = [i.smoothed_covariances_diagonal(m).numpy() + (s - mean) ** 2 for i, m, s in zip(self._inf, ppca._models, sm)]
        return Dataset(np.ascontiguousarray(self._weighted(dg)))

    def extrapolated_covariances(self, ppca: PPCAMix, dataset: Dataset) -> List[np.ndarray]:
        """mix.rs:464-477 -- as written upstream each component contributes its SMOOTHED covariance."""
        return self._cov_sum([i.extrapolated(m, dataset).numpy() for i, m in zip(self._inf, ppca._models)],
                             [i.smoothed_covariances(m) for i, m in zip(self._inf, ppca._models)])

    def extrapolated_covariances_diagonal(self, ppca: PPCAMix, dataset: Dataset) -> Dataset:
        """mix.rs:485-505"""
        ex = [i.extrapolated(m, dataset).numpy() for i, m in zip(self._inf, ppca._models)]
        mean = self._weighted(ex)
        dg = [i.extrapolated_covariances_diagonal(m, dataset).numpy() + (e - mean) ** 2
              for i, m, e in zip(self._inf, ppca._models, ex)]
        return Dataset(np.ascontiguousarray(self._weighted(dg)))

    def posterior_sampler(self) -> "PosteriorSamplerMix":
        """mix.rs:508-518"""
        return PosteriorSamplerMix(np.exp(self._lp), [i.posterior_sampler() for i in self._inf])


class PosteriorSamplerMix:
    """mix.rs:521-537; src/python_bindings.rs:887-905: a component per sample from its posterior, then a draw
    from that component's state posterior pushed through its model.  Host-side, with numpy's generator (its draws for a
    seed are kept as they are); PPCAMix.sample_posterior draws on the GPU in one call."""

    def __init__(self, posteriors: np.ndarray, samplers: List["PosteriorSampler"]):
        self._post, self._samplers = posteriors, samplers

    def sample(self, seed: Optional[int] = None) -> Dataset:
        rng = np.random.default_rng(seed)
        n = self._post.shape[0]
        p = self._post / self._post.sum(axis=1, keepdims=True)
        which = (rng.random((n, 1)) > np.cumsum(p, axis=1)).sum(axis=1).clip(0, p.shape[1] - 1)
        draws = [s.sample(seed=int(rng.integers(0, 2 ** 63 - 1))).numpy() for s in self._samplers]
        return Dataset(np.ascontiguousarray(np.stack(draws)[which, np.arange(n)]))


@dataclass
class PPCAMixTrainer:
    """python/ppca_rs/__init__.py:70-118"""

    dataset: Dataset

    def train(self, *, start: Optional[PPCAMix] = None, prior: Optional[Prior] = None, n_models: int,
              state_size: int, n_iters: int = 10, metric: Literal["aic", "bic", "llk"] = "aic", quiet: bool = False,
              seed: Optional[int] = None, init: str = "random") -> PPCAMix:
        """init: the `method` of `PPCAMix.init` when no `start` is given."""
        ds = self.dataset
        model = start or PPCAMix.init(n_models, state_size, ds, seed=seed, method=init)
        return _train_loop(model, n_iters, quiet, metric, "PPCA mix", len(ds), lambda m: m.iterate_with_llk(ds, prior),
                           lambda m: m.iterate_with_prior(ds, prior) if prior is not None else m.iterate(ds))


# --------------------------------------------------------------------------- mixture of factor analysers (shared column noise)
class FAMix:
    """Mixture of factor analysers with ONE noise level per column shared by all components (Ghahramani & Hinton):
    y | c = C_c x + mean_c + noise, x ~ N(0, I), noise_j ~ N(0, noise[j]^2), P(c) = weights[c] -- FAModel's per-column noise met with
    PPCAMix's mixture of subspaces (an extension with no reference counterpart; include/ppca_hip.h).  All components
    have the same state size.

    Every pass runs the PPCAMix kernels on the dataset with column j divided by noise[j] (`whitened()` is the mixture of that
    dataset): one whitened copy serves every component; it is made on the GPU for the call and released with it.
    """

    def __init__(self, noise, transforms, means, log_weights, *, ctx=None):
        t = np.array(transforms, dtype=np.float64, order="C")
        if t.ndim != 3 or t.shape[0] < 1:
            raise TypeError("transforms must be a 3-D float64 array (n_models, d, k)")
        m = np.array(means, dtype=np.float64, order="C")
        if m.ndim != 2:
            raise TypeError("means must be a 2-D float64 array (n_models, d)")
        if m.shape[0] != t.shape[0]:
            raise ValueError("transforms and means differ in the number of components")
        lw = f64(log_weights).ravel()
        if lw.shape[0] != t.shape[0]:
            raise ValueError("components and log_weights differ in length")
        first = FAModel(noise, t[0], m[0], ctx=ctx)  # (the checks of noise, transform and mean are FAModel's)
        self._noise, self._c, self._mean, self._ctx = first._noise, t, m, ctx
        self._lw = _log_softmax(lw)
        self._c.setflags(write=False)
        self._mean.setflags(write=False)

    # -- getters ----------------------------------------------------------------
    @property
    def noise(self) -> np.ndarray:
        return self._noise.copy()

    @property
    def transforms(self) -> np.ndarray:
        return self._c.copy()

    @property
    def means(self) -> np.ndarray:
        return self._mean.copy()

    @property
    def log_weights(self) -> np.ndarray:
        return self._lw.copy()

    @property
    def weights(self) -> np.ndarray:
        return np.exp(self._lw)

    @property
    def output_size(self) -> int:
        return int(self._c.shape[1])

    @property
    def state_size(self) -> int:
        return int(self._c.shape[2])

    @property
    def n_models(self) -> int:
        return int(self._c.shape[0])

    @property
    def n_parameters(self) -> int:
        """The shared noise, per component a transform and a mean, and the free weights."""
        d, k, nm = self.output_size, self.state_size, self.n_models
        return d + nm * (d * k + d) + nm - 1

    def __repr__(self) -> str:
        return f"FAMix(n_models={self.n_models}, output_size={self.output_size}, state_size={self.state_size}, noise=array({self._noise}))"

    # -- construction -------------------------------------------------------------
    @staticmethod
    def init(n_models: int, state_size: int, dataset: Dataset, seed: Optional[int] = None, method: str = "random") -> "FAMix":
        """The components of PPCAMix.init (same seed, same draws), noise = 1, equal weights.  method="kmeans":
        `from_kmeans(state_size, dataset, dataset.kmeans(n_models, seed=seed, scale="std"))` -- clustered in units of every column's
        own standard deviation, so that the whole start commutes with rescaling a column."""
        if method == "kmeans":
            return FAMix.from_kmeans(state_size, dataset, dataset.kmeans(n_models, seed=seed, scale="std"))
        if method != "random":
            raise ValueError("method must be 'random' or 'kmeans'")
        mix = PPCAMix.init(n_models, state_size, dataset, seed=seed)
        return FAMix(np.ones(mix.output_size), np.stack([m._c for m in mix._models]), np.stack([m._mean for m in mix._models]),
                     mix._lw)

    @staticmethod
    def from_kmeans(state_size: int, dataset: Dataset, km: "KMeans") -> "FAMix":
        """The k-means start: per cluster `FAModel.from_moments` of the cluster's rows (the moments of PPCAMix.from_kmeans, the same rule
        for a cluster of weight 0), weights as there; the shared noise pools the clusters' own, noise_j^2 = sum_c tot_cj noise_cj^2 /
        sum_c tot_cj with tot_cj the weight of cluster c's rows that observe column j (1 where no cluster observes the column)."""
        moms, whole, lw = _kmeans_cluster_moments(dataset, km)
        parts = [FAModel.from_moments(state_size, m if m is not None else whole) for m in moms]
        d = parts[0].output_size
        num, den = np.zeros(d), np.zeros(d)
        for m, f in zip(moms, parts):
            if m is not None:
                tot = np.diag(m._counts)
                num += tot * f._noise ** 2
                den += tot
        noise = np.where(den > 0.0, np.sqrt(num / np.where(den > 0.0, den, 1.0)), 1.0)
        return FAMix(noise, np.stack([f._c for f in parts]), np.stack([f._mean for f in parts]), lw)

    @staticmethod
    def from_ppca_mix(mix: PPCAMix) -> "FAMix":
        """The FA mixture equal to an isotropic one whose components share their noise level and state size."""
        if len({m.isotropic_noise for m in mix._models}) != 1 or len(set(mix.state_sizes)) != 1:
            raise ValueError("the components must share their isotropic noise and state size: the noise of an FAMix is shared")
        m0 = mix._models[0]
        return FAMix(np.full(m0.output_size, m0.isotropic_noise), np.stack([m._c for m in mix._models]),
                     np.stack([m._mean for m in mix._models]), mix._lw)

    @staticmethod
    def from_fa(models: Sequence[FAModel], log_weights) -> "FAMix":
        """From FA models that share their noise vector and state size."""
        models = list(models)
        if not models:
            raise ValueError("need at least one model")
        if any(m._c.shape != models[0]._c.shape or not np.array_equal(m._noise, models[0]._noise) for m in models):
            raise ValueError("the models must share their noise vector and shape: the noise of an FAMix is shared")
        return FAMix(models[0]._noise, np.stack([m._c for m in models]), np.stack([m._mean for m in models]), log_weights)

    def whitened(self) -> PPCAMix:
        """PPCAMix of PPCAModel(1, diag(1 / noise) C_c, mean_c / noise): the mixture of the dataset whose column j is divided by
        noise[j]."""
        return PPCAMix([PPCAModel(1.0, c / self._noise[:, None], m / self._noise, ctx=self._ctx) for c, m in zip(self._c, self._mean)],
                       self._lw)

    def components(self) -> List[FAModel]:
        return [FAModel(self._noise, c, m, ctx=self._ctx) for c, m in zip(self._c, self._mean)]

    def to_canonical(self) -> "FAMix":
        """The rotation of PPCAModel.to_canonical on every C_c; noise, means and weights are untouched."""
        return FAMix(self._noise, np.stack([PPCAModel(1.0, c, m).to_canonical()._c for c, m in zip(self._c, self._mean)]), self._mean,
                     self._lw)

    def sample(self, dataset_size: int, mask_prob: float, seed: Optional[int] = None) -> Dataset:
        """The whitened mixture's `sample` with column j multiplied by noise[j]."""
        return self.whitened().sample(dataset_size, mask_prob, seed)._scale_columns(self._noise)[0]

    # -- passes ---------------------------------------------------------------------
    def _whiten(self, dataset: Dataset, **kw):
        if dataset._d != self.output_size:
            raise ValueError(f"dataset has {dataset._d} dimensions but the model has output size {self.output_size}")
        _dense_only(dataset)  # (the mixture of factor analysers on row-compressed data is not built: DESIGN.md section 7)
        return dataset._scale_columns(1.0 / self._noise, **kw)

    def llks(self, dataset: Dataset) -> np.ndarray:
        """Per-sample log-likelihood: the whitened mixture's on the whitened rows minus the sum of ln noise[j] over the row's
        observed entries."""
        y, _, jac = self._whiten(dataset, l=np.log(self._noise), row_sums=True)
        return self.whitened().llks(y) - jac

    def llk(self, dataset: Dataset) -> float:
        """Weighted log-likelihood."""
        y, sums, _ = self._whiten(dataset, col_sums=True)
        return self.whitened().llk(y) - float(np.dot(sums[0], np.log(self._noise)))

    def heldout_score(self, train: Dataset, held: Dataset) -> "HeldOutScore":
        """PPCAMix.heldout_score of the whitened mixture on both parts whitened with the same scales, mapped back to the units of
        the data (FAModel.heldout_score)."""
        score = self.whitened().heldout_score(self._whiten(train)[0], self._whiten(held)[0])
        return _heldout_unwhiten(score, held, self._noise)

    def infer_cluster(self, dataset: Dataset) -> np.ndarray:
        """Log posteriors over the components (N, n_models): those of the whitened mixture on the whitened rows."""
        return self.whitened().infer_cluster(self._whiten(dataset)[0])

    def smooth(self, dataset: Dataset) -> Dataset:
        """Posterior-weighted sum of the components' C_c z + mean_c for every dimension."""
        sm = self.whitened().smooth(self._whiten(dataset)[0])  # (the whitened copy is released here)
        return sm._scale_columns(self._noise)[0]

    def extrapolate(self, dataset: Dataset) -> Dataset:
        """Observed values kept bit for bit, masked ones replaced by the smoothed value."""
        sm = self.whitened().smooth(self._whiten(dataset)[0])
        return dataset._fill_masked(sm, self._noise)

    def _iterate(self, dataset: Dataset, min_noise, want_llk: bool):
        ctx = dataset._ctx
        if len(dataset) == 0:
            raise ValueError("dataset is empty")
        d, k, nm = self.output_size, self.state_size, self.n_models
        if dataset._d != d:
            raise ValueError(f"dataset has {dataset._d} dimensions but the model has output size {d}")
        floor = None
        if min_noise is not None:
            floor = np.ascontiguousarray(np.broadcast_to(np.asarray(min_noise, dtype=np.float64), (d,)))
        n_out, c_out, m_out, lw_out = np.empty(d), np.empty((nm, d, k)), np.empty((nm, d)), np.empty(nm)
        llk = C.c_double(0.0)
        check(lib().ppca_famix_em_step(ctx.handle, dataset._h, d, k, nm, ptr(self._noise), ptr(self._c), ptr(self._mean), ptr(self._lw),
                                       ptr(floor), ptr(n_out), ptr(c_out), ptr(m_out), ptr(lw_out), C.byref(llk) if want_llk else None))
        return FAMix(n_out, c_out, m_out, lw_out, ctx=self._ctx), (llk.value if want_llk else None)

    def iterate(self, dataset: Dataset, min_noise=None) -> "FAMix":
        """One ECM iteration: responsibilities from this model; per component the transform, then the mean; then the shared noise
        from all components' residuals pooled; new weights.  The log-likelihood cannot decrease.  min_noise: a floor for the new
        noise, a number or one per column."""
        return self._iterate(dataset, min_noise, False)[0]

    def iterate_with_llk(self, dataset: Dataset, min_noise=None):
        """(next model, llk of THIS model) from the same pass."""
        return self._iterate(dataset, min_noise, True)

    # -- serialisation (own npz container) ----------------------------------------------
    def dump(self) -> bytes:
        return _npz_dump("ppca_rs_amd.FAMix", noise=self._noise, transforms=self._c, means=self._mean, log_weights=self._lw)

    @staticmethod
    def load(data: bytes) -> "FAMix":
        return _npz_load(data, "ppca_rs_amd.FAMix", "an FAMix",
                         lambda z: FAMix(z["noise"], z["transforms"], z["means"], z["log_weights"]))

    def __getstate__(self):
        return self.dump()

    def __setstate__(self, state):
        self.__dict__.update(FAMix.load(state).__dict__)

    def __getnewargs__(self):
        return (self.noise, self.transforms, self.means, self.log_weights)


@dataclass
class FAMixTrainer:
    """EM driver of FAMix: the loop and metrics of FATrainer."""

    dataset: Dataset

    def train(self, *, n_models: int, state_size: int, n_iters: int = 10, start: Optional[FAMix] = None,
              metric: Literal["aic", "bic", "llk"] = "aic", quiet: bool = False, seed: Optional[int] = None,
              min_noise_ratio: float = 1e-3, init: str = "random") -> FAMix:
        """min_noise_ratio: FATrainer's floor, ratio x the column's observed standard deviation.  init: the `method` of `FAMix.init`
        when no `start` is given."""
        ds = self.dataset
        model = start or FAMix.init(n_models, state_size, ds, seed=seed, method=init)
        floor = min_noise_ratio * np.sqrt(ds.column_stats()[2])
        return _train_loop(model, n_iters, quiet, metric, "FA mix", len(ds), lambda m: m.iterate_with_llk(ds, floor),
                           lambda m: m.iterate(ds, floor))
