"""Re-ranked candidate lists on the device (include/madtp_lists.h, csrc/lists.hip): what stage 2 of a two-stage retrieval leaves
behind - k_test (key, score) pairs per query row - ranked and ordered without the dense [n, nk] score matrix they stand for.

    cl = lists.CandidateLists(idx, val, nk)              # idx int64 [n,k] (-1 = an empty slot), val f32 [n,k], fill = -100.0
    rank_row, rank_tgt = cl.rank(tgt_ptr, tgt_idx)       # what retrieval_eval.rank_scores(cl.to_dense(), ...) returns
    best = cl.sorted();  first = cl.top(10)              # the contract order of madtp_search.h, empty slots last
    cl.validate()                                        # index range and duplicates, checked on the device (synchronises)

A list stands for the dense row "val of the slot that holds j, fill for a key in no slot"; no key may occur twice in a row.
1 <= k <= MAX_K.  Device tensors only: a CPU tensor raises, there is no fallback."""
import torch

from . import abi, hip

# the one declaration of the entry points; lib() is hip.load()'s handle with them set on it (no GPU needed)
SIGNATURES, DEFINES, lib = abi.bind("madtp_lists.h", "madtp_lists_abi_version")
ABI_VERSION = DEFINES["MADTP_LISTS_ABI_VERSION"]
MAX_K = DEFINES["MADTP_LISTS_MAX_K"]
MAX_TARGETS = DEFINES["MADTP_LISTS_MAX_TARGETS"]
MAX_NK = 2 ** 31 - 1


def _pair(idx, val):
    """the checks of a list's two tensors that need no device -> (n, k)"""
    if not torch.is_tensor(idx) or idx.dtype != torch.int64:
        raise ValueError(f"idx must be an int64 tensor, not {getattr(idx, 'dtype', type(idx).__name__)}")
    if not torch.is_tensor(val) or val.dtype != torch.float32:
        raise ValueError(f"val must be a float32 tensor, not {getattr(val, 'dtype', type(val).__name__)}")
    if idx.dim() != 2 or tuple(val.shape) != tuple(idx.shape) or idx.shape[0] < 1:
        raise ValueError(f"idx {tuple(idx.shape)} and val {tuple(val.shape)} must be two [n, k] tensors of one shape, n >= 1")
    if idx.device != val.device:
        raise ValueError(f"idx is on {idx.device}, val on {val.device}")
    n, k = idx.shape
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k} outside [1, {MAX_K}]")
    return n, k


def _rows(t, name):
    """a GPU tensor whose rows the kernels can read in place (unit stride within a row), else its contiguous copy -> (t, ld)"""
    if not t.is_cuda:
        raise ValueError(f"{name} is a CPU tensor: the kernels take device tensors only (no CPU fallback)")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _targets(tgt_ptr, tgt_idx, n):
    for t, name in ((tgt_ptr, "tgt_ptr"), (tgt_idx, "tgt_idx")):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 vector")
    if tgt_ptr.numel() != n + 1:
        raise ValueError(f"tgt_ptr has {tgt_ptr.numel()} entries for {n} rows")
    if n > 0 and tgt_idx.numel() > 0:
        per_row = tgt_ptr[1:] - tgt_ptr[:-1]
        most = int(per_row.max())  # (for device targets this synchronises)
        if most > MAX_TARGETS:
            raise ValueError(f"tgt_ptr: row {int(per_row.argmax())} has {most} targets, at most {MAX_TARGETS} are supported")
    for t, name in ((tgt_ptr, "tgt_ptr"), (tgt_idx, "tgt_idx")):
        if not t.is_cuda:
            raise ValueError(f"{name} is a CPU tensor: the kernels take device tensors only (no CPU fallback)")


def rank(idx, val, nk, fill, tgt_ptr, tgt_idx):
    """(rank_row int32 [n], rank_tgt int32 [n_targets]) of the CSR targets in the rows the lists stand for (madtp_lists_rank)."""
    n, k = _pair(idx, val)
    nk = _check_nk(nk)
    _targets(tgt_ptr, tgt_idx, n)
    (idx, ld_idx), (val, ld_val) = _rows(idx, "idx"), _rows(val, "val")
    if tgt_idx.numel() == 0:  # no ground truth at all: nothing to launch, every row ranks nk
        return torch.full((n,), nk, dtype=torch.int32, device=idx.device), torch.empty(0, dtype=torch.int32, device=idx.device)
    rank_row = torch.empty(n, dtype=torch.int32, device=idx.device)
    rank_tgt = torch.empty(tgt_idx.numel(), dtype=torch.int32, device=idx.device)
    with torch.cuda.device(idx.device):
        hip._check(lib().madtp_lists_rank(idx.data_ptr(), ld_idx, val.data_ptr(), ld_val, n, k, nk, float(fill), tgt_ptr.data_ptr(),
                                          tgt_idx.data_ptr(), rank_row.data_ptr(), rank_tgt.data_ptr(), hip._stream()),
                   "madtp_lists_rank")
    return rank_row, rank_tgt


def sort(idx, val, nk):
    """(idx int64 [n,k], val f32 [n,k]) of every row, best first in the order of madtp_search.h (madtp_lists_sort)."""
    n, k = _pair(idx, val)
    nk = _check_nk(nk)
    (idx, ld_idx), (val, ld_val) = _rows(idx, "idx"), _rows(val, "val")
    out_idx = torch.empty(n, k, dtype=torch.int64, device=idx.device)
    out_val = torch.empty(n, k, dtype=torch.float32, device=idx.device)
    with torch.cuda.device(idx.device):
        hip._check(lib().madtp_lists_sort(idx.data_ptr(), ld_idx, val.data_ptr(), ld_val, n, k, nk, out_idx.data_ptr(),
                                          out_val.data_ptr(), hip._stream()), "madtp_lists_sort")
    return out_idx, out_val


def _check_nk(nk):
    nk = int(nk)
    if not 1 <= nk <= MAX_NK:
        raise ValueError(f"nk = {nk} outside [1, 2^31 - 1]")
    return nk


class CandidateLists:
    """idx int64 [n, k] and val f32 [n, k] over nk keys: row r stands for the dense row s_j = val[r, slot holding j], s_j = fill for
    a key in no slot.  idx == -1 marks an empty slot (its value is ignored); no key may occur twice in a row (validate()).  The
    tensors are kept as given, views included."""

    def __init__(self, idx, val, nk, fill=-100.0):
        _pair(idx, val)
        self.idx, self.val, self.nk, self.fill = idx, val, _check_nk(nk), float(fill)

    @property
    def shape(self):
        return tuple(self.idx.shape)

    @property
    def device(self):
        return self.idx.device

    @property
    def nbytes(self):
        """bytes of the two [n, k] tensors (not of the storage a view sits in)"""
        return self.idx.numel() * self.idx.element_size() + self.val.numel() * self.val.element_size()

    def rank(self, tgt_ptr, tgt_idx):
        """(rank_row, rank_tgt) as retrieval_eval.rank_scores(self.to_dense(), tgt_ptr, tgt_idx) gives them; no row is formed"""
        return rank(self.idx, self.val, self.nk, self.fill, tgt_ptr, tgt_idx)

    def sorted(self):
        """a new CandidateLists, every row best first: value descending, equal values by key descending, NaN below every number,
        empty slots last as (-1, -inf)"""
        return CandidateLists(*sort(self.idx, self.val, self.nk), self.nk, self.fill)

    def top(self, r):
        """the first r columns of sorted()"""
        r = int(r)
        if not 1 <= r <= self.idx.shape[1]:
            raise ValueError(f"r = {r} outside [1, k = {self.idx.shape[1]}]")
        s = self.sorted()
        return CandidateLists(s.idx[:, :r], s.val[:, :r], self.nk, self.fill)

    def to_dense(self):
        """the f32 [n, nk] matrix the lists stand for (a torch scatter): for tests and for callers of the dense return value"""
        n, k = self.idx.shape
        held = (self.idx >= 0) & (self.idx < self.nk)
        dense = torch.full((n, self.nk + 1), self.fill, dtype=torch.float32, device=self.idx.device)
        dense.scatter_(1, torch.where(held, self.idx, torch.full_like(self.idx, self.nk)), self.val)  # (empty slots: a spare column)
        return dense[:, :self.nk].contiguous()

    def validate(self):
        """ValueError naming the first row that holds an index outside {-1} + [0, nk) or a key twice.  Runs on the device the
        lists are on and synchronises."""
        bad = ((self.idx < -1) | (self.idx >= self.nk)).any(dim=1)
        keys = torch.sort(self.idx, dim=1).values
        twice = ((keys[:, 1:] == keys[:, :-1]) & (keys[:, 1:] >= 0)).any(dim=1)
        rows = torch.nonzero(bad | twice).flatten()
        if rows.numel():
            r = int(rows[0])
            if bool(bad[r]):
                j = self.idx[r][(self.idx[r] < -1) | (self.idx[r] >= self.nk)][0]
                raise ValueError(f"idx: row {r} holds index {int(j)} outside [0, {self.nk}) (and not -1)")
            j = keys[r, 1:][(keys[r, 1:] == keys[r, :-1]) & (keys[r, 1:] >= 0)][0]
            raise ValueError(f"idx: row {r} holds key {int(j)} twice")
        return self

    def to(self, device):
        return CandidateLists(self.idx.to(device), self.val.to(device), self.nk, self.fill)

    def cpu(self):
        return self.to("cpu")
