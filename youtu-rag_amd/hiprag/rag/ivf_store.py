"""``index_type: "IVF_FLAT"`` behind HipVectorStore: an exact index plus an IVF replica.

``IvfStoreIndex`` has the ``NativeIndex`` surface the store uses (add, add_device, remove, search, get_rows, save,
load, size, reserve, close) and plugs into the store's ``index_factory`` / ``index_loader`` seam.  It deliberately
has no ``search_device``, ``search_submit_host`` or ``devices``: the store's ``hasattr`` checks then send every batch
through the worker-thread path, which calls ``search(q, k, mask)``.

It owns the exact ``NativeIndex`` in append order -- the source of truth for row numbers, ``get_by_id``,
persistence and every exact answer, unchanged -- and beside it an ``IvfIndex`` replica (hiprag/ivf.py) whose ids are
the store's row numbers.  The replica holds a second copy of the rows: 50M x 1024 f16 is 102 GB + 102 GB of HBM.

Below ``ivf_train_rows`` live rows every search is exact.  The add that reaches the threshold trains the coarse
quantizer on a strided sample of the stored rows and places every live row with ``add_from`` (stored bits copied);
later adds feed both structures from the same raw vectors.  Nothing retrains by itself: ``rebuild_ivf()`` does.
``k > 1024``, ``nprobe >= nlist`` and an untrained replica are answered by the exact index.
"""
from __future__ import annotations

import logging
import os

import numpy as np

from .. import _native

logger = logging.getLogger(__name__)

IVF_MAX_K = 1024  # hr_ivf_search's largest k


def wants_ivf(index_type, metric: str, devices) -> bool:
    """Whether a store with this ``VectorStoreConfig.index_type`` is served by IVF lists.  "IVF_FLAT" (any letter
    case): yes -- single device and cosine / dot only, else ValueError.  None, "FLAT", "HNSW" and anything else: the
    exact store (one log line for a name the store does not know)."""
    name = (index_type or "").strip().upper()
    if name == "IVF_FLAT":
        if len(list(devices or [0])) > 1:
            raise ValueError('index_type "IVF_FLAT" needs a single-device store (index_params.devices has several)')
        if metric in ("l2", "euclidean"):
            raise ValueError('index_type "IVF_FLAT" supports the cosine and dot metrics, not euclidean')
        return True
    if name not in ("", "FLAT", "HNSW"):
        logger.info("index_type %r is not known to the HIP store: serving exact search", index_type)
    return False


class _DevRows:
    """n x dim fp32 rows at a raw device pointer, for torch.as_tensor (no copy)."""

    def __init__(self, ptr: int, n: int, dim: int):
        self.__cuda_array_interface__ = {"shape": (n, dim), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class IvfStoreIndex:
    def __init__(self, dim: int, dtype: str, metric: str, device: int = 0, nlist: int = 1024, nprobe: int = 16,
                 train_rows: int | None = None, seed: int = 0, _exact=None):
        self.dim, self.dtype, self.metric, self.device = int(dim), dtype, metric, int(device)
        self.nlist, self.nprobe, self.seed = int(nlist), int(nprobe), int(seed)
        if self.nlist < 1 or self.nprobe < 1:
            raise ValueError("index_params nlist and nprobe must be >= 1")
        self.train_rows = max(self.nlist, int(train_rows) if train_rows is not None else 64 * self.nlist)
        self.exact = _exact if _exact is not None else _native.NativeIndex(self.dim, dtype, metric, self.device)
        self.ivf = None                   # the trained replica
        self._live = np.zeros(0, bool)    # per store row; None: unknown (a snapshot without the side file)

    # ---------------------------------------------------------------- helpers
    def _torch(self):
        import torch

        return torch, torch.device("cuda", self.device)

    @property
    def trained(self) -> bool:
        return self.ivf is not None

    @property
    def centroids(self):
        """(nlist, dim) fp32 host centroids of the trained replica (None before training)."""
        return None if self.ivf is None else self.ivf.centroids[:, : self.dim].cpu().numpy()

    @property
    def lists_of_rows(self) -> np.ndarray:
        """List of every store row (host int64, -1: dead or not placed)."""
        n = self.exact.size()[0]
        out = np.full(n, -1, np.int64)
        if self.ivf is not None:
            got = self.ivf.lists_of_rows.cpu().numpy()
            out[: len(got)] = got[:n]
        return out

    def _mark(self, first: int, n: int):
        if self._live is None:
            return
        if len(self._live) < first + n:
            live = np.zeros(max(first + n, 2 * len(self._live), 1024), bool)
            live[: len(self._live)] = self._live
            self._live = live
        self._live[first:first + n] = True

    def _after_add(self, first: int, n: int, rows_dev):
        """rows_dev: the (n, dim) fp32 device tensor the exact index just stored as rows [first, first + n)."""
        self._mark(first, n)
        if self.ivf is not None:
            self.ivf.add(rows_dev, np.arange(first, first + n, dtype=np.int64))
        elif self._live is not None and self.exact.size()[1] >= self.train_rows:
            self.rebuild_ivf()

    def rebuild_ivf(self, live_rows=None):
        """Train a fresh replica on a strided sample of the stored live rows and place every live row in it
        (``live_rows``: the store's own list, needed only after loading a snapshot without the side file)."""
        from ..ivf import IvfIndex

        torch, dev = self._torch()
        n = self.exact.size()[0]
        if live_rows is not None:
            self._live = np.zeros(max(n, 1024), bool)
            self._live[np.asarray(live_rows, np.int64)] = True
        if self._live is None:
            raise RuntimeError("the live rows are unknown: pass live_rows")
        rows = np.nonzero(self._live[:n])[0].astype(np.int64)
        if len(rows) < self.nlist:
            raise ValueError(f"{len(rows)} live rows cannot train {self.nlist} lists")
        sample = rows[:: max(1, len(rows) // max(self.train_rows, 64 * self.nlist))]
        ivf = IvfIndex(self.dim, self.nlist, dtype=self.dtype, metric=self.metric, device=self.device)
        ivf.train(torch.from_numpy(self.exact.get_rows(sample)).to(dev), seed=self.seed)
        ivf.add_from(self.exact, rows)
        old, self.ivf = self.ivf, ivf
        if old is not None:
            old.close()
        logger.info("IVF replica trained: %d lists over %d rows", self.nlist, len(rows))

    # ---------------------------------------------------------------- the NativeIndex surface
    def reserve(self, rows: int):
        self.exact.reserve(rows)

    def size(self):
        return self.exact.size()

    def get_rows(self, rows):
        return self.exact.get_rows(rows)

    def add(self, rows: np.ndarray) -> int:
        torch, dev = self._torch()
        rows = np.ascontiguousarray(rows, np.float32)
        first = self.exact.add(rows)
        if len(rows):
            self._after_add(first, len(rows), torch.tensor(rows, device=dev) if self.ivf is not None else None)
        return first

    def add_device(self, rows_ptr: int, n: int, stream: int = 0) -> int:
        torch, dev = self._torch()
        first = self.exact.add_device(rows_ptr, n, stream)
        if not n:
            return first
        if self.ivf is None:
            self._after_add(first, n, None)
            return first
        # the same raw vectors into the replica, ordered on the caller's stream like the exact add
        ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)) if stream else torch.cuda.device(dev)
        with ctx:
            self._after_add(first, n, torch.as_tensor(_DevRows(rows_ptr, n, self.dim), device=dev))
        return first

    def remove(self, rows) -> None:
        rows = np.asarray(rows, np.int64).reshape(-1)
        self.exact.remove(rows)
        if self._live is not None:
            self._live[rows[rows < len(self._live)]] = False
        if self.ivf is not None:
            self.ivf.remove(rows)

    def search(self, q: np.ndarray, k: int, mask: np.ndarray | None = None):
        ivf = self.ivf
        if ivf is None or k > IVF_MAX_K or self.nprobe >= self.nlist:
            return self.exact.search(q, k, mask)
        torch, dev = self._torch()
        q = np.ascontiguousarray(q, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != index dim {self.dim}")
        with torch.cuda.device(dev):
            qd = torch.from_numpy(q).to(dev)
            B = q.shape[0]
            cand = torch.empty((B, k, 2), dtype=torch.float64, device=dev)
            bound = torch.empty(B, dtype=torch.float64, device=dev)
            mask_ptr, keep = 0, None
            if mask is not None:
                words = np.ascontiguousarray(mask, np.uint64).reshape(-1)
                md = torch.from_numpy(words.view(np.int64)).to(dev)
                npos = ivf.n_positions
                pm = torch.empty((npos + 31) // 32, dtype=torch.int32, device=dev)
                st = torch.cuda.current_stream(dev).cuda_stream
                _native.ivf_position_mask(ivf.ids.data_ptr(), npos, md.data_ptr(), len(words) * 64, pm.data_ptr(), st)
                mask_ptr, keep = pm.data_ptr(), (md, pm)
            ivf.search_candidates(qd, k, self.nprobe, cand, bound, mask_ptr=mask_ptr)
            host = cand.cpu().numpy()  # one copy back (after the search, on the same stream): {score f64, id i64}
            del keep
        return host[..., 0].astype(np.float32), host.view(np.int64)[..., 1].copy()

    # collapsed search (one hit per group) is always exact: the exact index holds the group column and answers
    def set_groups(self, row0: int, groups) -> None:
        self.exact.set_groups(row0, groups)

    def search_collapsed(self, q: np.ndarray, k: int, mask: np.ndarray | None = None, probe: int = 0):
        return self.exact.search_collapsed(q, k, mask, probe)

    def collapse_stats(self) -> dict:
        return self.exact.collapse_stats()

    # MMR search is always exact too: its pool is the exact top-fetch_k, so the exact index answers
    def search_mmr(self, q: np.ndarray, k: int, lam: float, mask: np.ndarray | None = None, fetch_k: int = 0):
        return self.exact.search_mmr(q, k, lam, mask, fetch_k)

    # a range answer is exact by definition (every row at or above the threshold): the exact index answers
    def search_range(self, q: np.ndarray, min_score, max_hits: int = 1024, mask: np.ndarray | None = None):
        return self.exact.search_range(q, min_score, max_hits, mask)

    def range_stats(self) -> dict:
        return self.exact.range_stats()

    # a boosted answer is exact over the whole collection by definition: the exact index holds the boost columns
    def set_boost(self, col: int, row0: int, values) -> None:
        self.exact.set_boost(col, row0, values)

    def search_boosted(self, q: np.ndarray, k: int, alpha: float, betas, mask: np.ndarray | None = None,
                       probe: int = 0, window: int = 0):
        return self.exact.search_boosted(q, k, alpha, betas, mask, probe, window)

    def boost_stats(self) -> dict:
        return self.exact.boost_stats()

    # ---------------------------------------------------------------- persistence
    def save(self, path: str) -> None:
        """The exact index to ``path`` as ever, and ``path + ".ivf.npz"``: centroids, nlist, the seed, the list of
        every row and the live rows (written first: the index file completes the pair)."""
        n = self.exact.size()[0]
        live = np.zeros(n, bool) if self._live is None else self._live[:n].copy()
        if self._live is not None and len(live) < n:
            live = np.concatenate([live, np.zeros(n - len(live), bool)])
        cent = self.ivf.centroids.cpu().numpy() if self.ivf is not None else np.zeros((0, 0), np.float32)
        side = path + ".ivf.npz"
        with open(side + ".tmp", "wb") as f:
            np.savez(f, centroids=cent, lists=self.lists_of_rows, live=np.packbits(live),
                     meta=np.array([self.nlist, self.seed, n, int(self.ivf is not None),
                                    int(self._live is not None)], np.int64))
            f.flush()
            os.fsync(f.fileno())
        os.replace(side + ".tmp", side)
        self.exact.save(path)

    @classmethod
    def load(cls, path: str, dim: int, dtype: str, metric: str, device: int = 0, nlist: int = 1024, nprobe: int = 16,
             train_rows: int | None = None, seed: int = 0) -> "IvfStoreIndex":
        from ..ivf import IvfIndex

        exact = _native.NativeIndex.load(path, device=device, dim=dim, dtype=dtype, metric=metric)
        self = cls(exact.dim, exact.dtype, exact.metric, device, nlist, nprobe, train_rows, seed, _exact=exact)
        n = exact.size()[0]
        side = path + ".ivf.npz"
        if not os.path.exists(side):
            # a snapshot written by an exact store: which rows are live is the store's knowledge
            logger.warning("%s has no IVF side file: exact search until rebuild_ivf()", path)
            self._live = None
            return self
        z = np.load(side, allow_pickle=False)
        nl, sd, n_side, trained, live_known = (int(v) for v in z["meta"])
        if n_side != n:
            raise RuntimeError(f"{side} describes {n_side} rows, the index holds {n}")
        self._live = np.unpackbits(z["live"], count=n).astype(bool) if live_known else None
        if trained and nl == self.nlist:
            import torch

            lists = z["lists"].astype(np.int64)
            rows = np.nonzero(lists >= 0)[0].astype(np.int64)
            ivf = IvfIndex(exact.dim, nl, dtype=exact.dtype, metric=exact.metric, device=device)
            ivf.centroids = torch.from_numpy(z["centroids"]).to(ivf.dev).contiguous()
            ivf.add_from(exact, rows, lists=lists[rows])
            self.ivf = ivf
        elif trained and self._live is not None:  # another nlist in the config: train anew
            self.rebuild_ivf()
        return self

    def close(self):
        if self.ivf is not None:
            self.ivf.close()
            self.ivf = None
        if self.exact is not None:
            self.exact.close()
