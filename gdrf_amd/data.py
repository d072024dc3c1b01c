"""Synthetic GDRF workloads and the reference's CSV normalisation.

``synth_circles`` follows the recipe of the reference's ``generate_data_2d_circles``
(gdrf/models/utils.py:106-193: one-topic discs over a uniform background, Girdhar-style
block word distributions, U{V..10V-1} words per cell), vectorised with numpy so that the
N = 1e6 benchmark lattice is generated in seconds.  ``normalise_index`` is the index -> [0,1]^D
map of gdrf/train_script.py:261-267.

Sparse counts: ``to_csr`` / ``csr_rows`` build and cut ``torch.sparse_csr`` count matrices (torch cannot index one by rows), and
``check_counts`` is the validation every entry point that reads counts applies, dense or CSR.
"""
from __future__ import annotations

import numpy as np


def normalise_index(index: np.ndarray) -> np.ndarray:
    index = np.asarray(index, dtype=np.float64)
    if index.ndim == 1:
        index = index[:, None]
    index = index - index.min(axis=0, keepdims=True)
    return index / index.max(axis=0, keepdims=True)


def synth_circles(W: int, H: int, V: int, K: int, *, n_discs=8, R_frac=0.1, eta=0.1, seed=777,
                  one_d: bool = False):
    """Regular lattice xs in [0,1]^D (train_script.py:261-267 normalisation), K-1 disc
    topics over a uniform background, per-cell total count ~ U{V..10V-1}, ws ~ Multinomial."""
    rng = np.random.default_rng(seed)
    if one_d:
        N = W
        idx = np.arange(N, dtype=np.float64)[:, None]
        xs = idx / idx.max()
        centers = rng.uniform(0.1, 0.9, size=(n_discs, 1))
    else:
        gx, gy = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
        idx = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64)
        xs = idx / idx.max(0, keepdims=True)
        centers = rng.uniform(0.1, 0.9, size=(n_discs, 2))
    N = xs.shape[0]
    K_obj = K - 1
    obj_topics = rng.integers(0, K_obj, size=n_discs) if K_obj > 0 else np.full(n_discs, K - 1)
    p_v_z = np.full((K, V), eta)
    for k in range(K_obj):
        lo, hi = V * k / K_obj, V * (k + 1) / K_obj
        vs = np.arange(V)
        p_v_z[k, (vs >= lo) & (vs < hi)] += 1.0
    p_v_z[K - 1, :] = 1.0 / V
    p_v_z /= p_v_z.sum(-1, keepdims=True)
    topic = np.full(N, K - 1)
    for i in range(n_discs - 1, -1, -1):
        d2 = ((xs - centers[i]) ** 2).sum(-1)
        topic[d2 <= R_frac * R_frac] = obj_topics[i]
    counts = rng.integers(V, 10 * V, size=N)
    ws = np.empty((N, V), dtype=np.int32)
    for k in range(K):
        sel = np.nonzero(topic == k)[0]
        if sel.size:
            ws[sel] = rng.multinomial(counts[sel], p_v_z[k]).astype(np.int32)
    return xs.astype(np.float32), ws, topic


# ---- sparse (CSR) count matrices ---------------------------------------------------------------------------------------------------
def is_sparse_counts(ws) -> bool:
    """True for a torch tensor in any sparse layout."""
    import torch
    return isinstance(ws, torch.Tensor) and ws.layout != torch.strided


def to_csr(dense):
    """An (n, V) array or dense tensor of counts as a ``torch.sparse_csr`` tensor with int32 values and int64 indices, on the same device."""
    import torch
    d = torch.as_tensor(dense)
    if d.dim() != 2:
        raise ValueError(f"to_csr: counts must be 2-d (n, V), got shape {tuple(d.shape)}")
    return mark_checked(d.to(torch.int32).to_sparse_csr())          # built here from a dense array: well formed by construction


# What this module records about a CSR tensor lives in ONE attribute of the tensor object, a dict keyed on the tensor's ``_version`` (as
# the engine's per-tensor caches are): {"version", "checked", "crow_host"}.  torch drops attributes in .to() / clone(): csr_to carries it.
def _meta(ws) -> dict:
    m = getattr(ws, "_gdrf_csr", None)
    if m is None or m["version"] != ws._version:
        m = ws._gdrf_csr = dict(version=ws._version, checked=False, crow_host=None)
    return m


def mark_checked(ws):
    """Declare the CSR tensor ``ws`` well formed (row pointers from 0 to nnz, not decreasing; column indices in [0, V)), so that
    ``check_counts`` skips the index checks that read from the device.  For matrices built well formed by construction.  Returns ``ws``."""
    _meta(ws)["checked"] = True
    return ws


def is_checked(ws) -> bool:
    return bool(_meta(ws)["checked"])


def csr_to(ws, device):
    """The CSR tensor ``ws`` on ``device`` (itself when it is there already), keeping what this module recorded about it."""
    import torch
    if ws.device == torch.device(device):
        return ws
    out = ws.to(device)
    out._gdrf_csr = dict(_meta(ws), version=out._version)
    return out


def _crow_host(ws):
    """The row pointers of a CSR tensor as a numpy int64 array, read from the device once per tensor object and ``_version``."""
    m = _meta(ws)
    if m["crow_host"] is None:
        m["crow_host"] = ws.crow_indices().detach().to("cpu").numpy().astype(np.int64)
    return m["crow_host"]


def csr_rows(ws, sel):
    """Rows ``sel`` of the CSR tensor ``ws`` as a new CSR tensor on the same device: ``sel`` a slice, an int, or a 1-d array of row indices
    (any order, repeats allowed, may be empty).  Built from the index arrays; the row pointers are kept on the host after their first
    read, so cutting rows from the same matrix again waits for no device work.  What is cut from a validated matrix counts as validated."""
    import torch
    if not isinstance(ws, torch.Tensor) or ws.layout != torch.sparse_csr:
        raise ValueError("csr_rows: ws must be a torch.sparse_csr tensor")
    n, V = ws.shape
    crow = _crow_host(ws)
    col, val = ws.col_indices(), ws.values()
    if isinstance(sel, slice) and (sel.step is None or sel.step == 1):
        a, b, _ = sel.indices(n)
        b = max(a, b)
        lo, hi = int(crow[a]), int(crow[b])
        new_crow = crow[a:b + 1] - crow[a]
        new_col, new_val = col[lo:hi].clone(), val[lo:hi].clone()
    else:
        if isinstance(sel, slice):
            sel = np.arange(n)[sel]
        if isinstance(sel, torch.Tensor):
            sel = sel.detach().cpu().numpy()
        idx = np.atleast_1d(np.asarray(sel)).astype(np.int64).reshape(-1)
        if idx.size and (idx.min() < -n or idx.max() >= n):
            raise IndexError(f"csr_rows: row index outside [0, {n})")
        idx = np.where(idx < 0, idx + n, idx)
        starts, lens = crow[idx], crow[idx + 1] - crow[idx]
        new_crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        # position of every kept entry in the source: its row's start plus its offset inside the row
        pos = np.repeat(starts - new_crow[:-1], lens) + np.arange(int(new_crow[-1]), dtype=np.int64)
        pos_t = torch.from_numpy(pos).to(col.device)
        new_col, new_val = col[pos_t], val[pos_t]
    new_crow = np.ascontiguousarray(new_crow, dtype=np.int64)
    out = torch.sparse_csr_tensor(torch.from_numpy(new_crow).to(device=col.device, dtype=ws.crow_indices().dtype), new_col, new_val,
                                  size=(len(new_crow) - 1, V))
    out._gdrf_csr = dict(version=out._version, checked=is_checked(ws), crow_host=new_crow)
    return out


def check_counts(ws, n=None, V=None, device=None):
    """Validate a count matrix: a dense (n, V) int32 tensor, or a ``torch.sparse_csr`` one with int32 values and int32 / int64 indices.
    Raises ValueError naming the offending property (layout, shape, dtype, device, crow_indices, col_indices); ``n``, ``V`` and ``device``
    are checked when given.  Needs no device context.  The index checks of a CSR matrix read from the device, so they run once per tensor
    object (and not at all for what ``to_csr`` and ``csr_rows`` built from a checked one)."""
    import torch
    if not isinstance(ws, torch.Tensor):
        raise ValueError("ws must be a torch tensor")
    if ws.layout not in (torch.strided, torch.sparse_csr):
        raise ValueError(f"ws layout must be torch.strided or torch.sparse_csr, got layout {ws.layout} (COO and CSC inputs are not supported: "
                         "convert with .to_sparse_csr())")
    if ws.dim() != 2 or (n is not None and ws.shape[0] != n) or (V is not None and ws.shape[1] != V):
        raise ValueError(f"ws shape must be ({'n' if n is None else n}, {'V' if V is None else V}), got shape {tuple(ws.shape)}")
    dt = ws.dtype if ws.layout == torch.strided else ws.values().dtype
    if dt != torch.int32:
        raise ValueError(f"ws dtype must be torch.int32, got dtype {dt}")
    if device is not None and ws.device != torch.device(device):
        raise ValueError(f"ws device must be {device}, got device {ws.device}")
    if ws.layout == torch.strided:
        if not ws.is_contiguous():
            raise ValueError("ws must be contiguous")
        return
    crow, col = ws.crow_indices(), ws.col_indices()
    if crow.dtype not in (torch.int32, torch.int64) or col.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ws index dtype must be torch.int32 or torch.int64, got {crow.dtype} / {col.dtype}")
    if ws.values().dim() != 1 or crow.dim() != 1:
        raise ValueError("ws shape: batched or blocked CSR tensors are not supported")
    if is_checked(ws):
        return
    nnz = int(col.shape[0])
    ch = _crow_host(ws)
    if ch.shape[0] != ws.shape[0] + 1 or ch[0] != 0 or ch[-1] != nnz:
        raise ValueError(f"ws crow_indices must hold n + 1 values that start at 0 and end at nnz = {nnz}, got "
                         f"{ch.shape[0]} values from {int(ch[0]) if ch.size else None} to {int(ch[-1]) if ch.size else None}")
    if (np.diff(ch) < 0).any():
        raise ValueError("ws crow_indices must not decrease")
    if nnz:
        lo, hi = (int(x) for x in torch.stack([col.min(), col.max()]).cpu())
        if lo < 0 or hi >= ws.shape[1]:
            raise ValueError(f"ws col_indices must lie in [0, {ws.shape[1]}), got values from {lo} to {hi}")
    mark_checked(ws)
