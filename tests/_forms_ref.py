"""A plain Python restatement of the rules by which the library picks a kernel form per stage from K, Mp, n and the context's modes
(gdrf_amd/csrc/forms.h; the slots of gdrf_last_forms, include/gdrf_hip.h).  CPU only: it imports neither the engine nor the oracle.

It was written from the launch code as it stood before the rules moved into forms.h, condition for condition and in that code's nesting, so
that tests/test_forms_host.py compares two statements of the rules that do not share a line: this one and the table that
tests/host/forms_table.cpp prints from forms.h.  ``forms(shape)`` gives, for a fresh context after one step on n rows and one
gdrf_predict(predict_mode) on n rows, the 17 slots by Engine.FORM_SLOTS' names as numbers (0: the stage did not run, or refused the shape)
and the split counts of A_k (ns, nst, ns1), G^T (gt_ns) and the hyper-TN form (hyper_ns).  ``resolve`` turns Engine's keywords into a shape
the way Engine.__init__ and gdrf_ctx_create_ex do.

``mm_plan`` (the M x M products of step_finish, slots mm_chain and mm_sbar) was written from Impl::mm_nt's own condition; ``mm_plan_old`` keeps
the rule as it stood while Sbar_k = 2 A_k S_k could share the slab buffer with the Cholesky-backward chain (a single product splits,
whichever stream it runs on), as the simulated fault of tests/test_forms_host.py.
"""
import functools
import math

TILE, MPAD, DMAX, KMAX, LOC_KMAX, TNT_KT, TN1_CH = 128, 32, 4, 32, 16, 10, 64      # csrc/common.h, kernels_n.h, gemm_tn_topics.h, gemm_tn_topics1.h
IMG = {1: 3 * 128 * 32, 2: 2 * 128 * 32}       # halfwords per operand image: bf16x6 (three pieces), f16x3 (two)
W1_WIMG = 4 * 128 * 32 * 2
FWD_T_W1_KGP = 2
KB = 1024
KINDS = ("rbf", "matern52", "matern32", "exponential", "rationalquadratic")
FIELDS = ("n", "n_cap", "M", "K", "V", "D", "esz", "ssz", "split", "stored_t", "rows_form", "csr", "hyper_tn", "learn_z", "ard", "per", "kind",
          "predict_mode", "unwhitened")
EXTRA = ("ns", "nst", "ns1", "gt_ns", "hyper_ns")


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


@functools.lru_cache(maxsize=None)
def tn_nsplit(K, nt, n, BR, wg_per_cu=3):
    tiles = K * nt * (nt + 1) // 2
    slots = 256.0 * wg_per_cu
    maxs = max(1, min(64, cdiv(n, 8 * BR)))
    best, best_eff = 1, 0.0
    for ns in range(1, maxs + 1):
        rounds = tiles * float(ns) / slots
        eff = rounds / math.ceil(rounds)
        if eff > best_eff + 1e-9 or (eff > best_eff - 0.02 and rounds >= 2.0 and tiles * float(best) / slots < 2.0):
            best_eff, best = eff, ns
    return best


@functools.lru_cache(maxsize=None)
def tn_nsplit_gt(K, nt, n, BR):
    maxs = min(64, cdiv(n, 8 * BR))
    if maxs < 8:
        return tn_nsplit(K, nt, n, BR, 2)
    tiles = nt * nt
    best, best_eff = 8, 0.0
    for ns in range(8, maxs + 1, 8):
        rounds = tiles * float(ns) / 512.0
        eff = rounds / math.ceil(rounds)
        if eff > best_eff + 1e-9 or (eff > best_eff - 0.02 and rounds >= 2.0 and tiles * float(best) / 512.0 < 2.0):
            best_eff, best = eff, ns
    return best


def tnt_ntiles(ncols):
    nI, nJ = cdiv(ncols, 128), cdiv(ncols, 64)
    return sum(min(2 * I + 2, nJ) for I in range(nI))


@functools.lru_cache(maxsize=None)
def tn_topics_nsplit(K, Mp, n):
    units = tnt_ntiles(Mp) * cdiv(K, TNT_KT)
    maxs = max(1, min(64, cdiv(n, 16 * 32)))
    chunk_us = 3.7
    slab_us_per_split = 2.0 * float(K) * Mp * Mp * 4.0 / 5.0e6
    best, best_t = 1, 1e300
    for ns in range(1, maxs + 1):
        rounds = math.ceil(units * float(ns) / 256.0)
        t = rounds * math.ceil(float(n) / (32.0 * ns)) * chunk_us + ns * slab_us_per_split
        if t < best_t * 0.995:
            best_t, best = t, ns
    return best


def nsplit_cap(K, Mp, n_cap, esz):
    nt = cdiv(Mp, TILE)
    cap = tn_nsplit(K, nt, n_cap, 128 // esz)
    if esz == 4:
        cap = max(cap, tn_nsplit(K, nt, n_cap, 32, 2), tn_nsplit_gt(K, nt, n_cap, 32), 64)
    return cap


def hyper_tn_on(s, Mp):
    return bool(s["hyper_tn"] and s["split"] == 2 and s["ssz"] == 8 and not s["learn_z"] and not s["ard"] and not s["per"]
                and s["kind"] != KINDS.index("rationalquadratic") and not s["stored_t"] and Mp // 8 <= 256)


def _wbar(s, Mp, cap):
    """(form, nslice); (0, 0) where the split form refuses the shape"""
    n, K = s["n"], s["K"]
    if s["stored_t"]:
        return 2, 1
    if not s["split"]:
        return 1, 1
    f16, img = s["split"] == 2, IMG[s["split"]]
    tabb = (K * TILE * 4 + 15) & ~15
    grp = 2 * img * 2 + tabb
    rtiles, nct = cdiv(n, TILE), cdiv(Mp, TILE)
    if K >= 2 and 2 * grp <= 160 * KB:
        pairs = (rtiles + 1) // 2
        lds_cc = 6 * img * 2 + 2 * tabb
        if f16 and K >= 2 and Mp % 64 == 0 and 8 * img * 2 + 2 * tabb <= 160 * KB:
            nkb = Mp // 64
            if pairs * nct > 32 and K <= 16:
                return 7, 1
            nslice = 1
            if pairs * nct <= 32 and nkb >= 2:
                nslice = min(nkb, 8)
            if nslice * round_up(n, 256) * Mp > cap * (K + 1) * Mp * Mp:
                nslice = 1
            return 6, nslice
        if lds_cc <= 160 * KB:
            return 5, 1
        return 4, 1
    if grp > 160 * KB:
        return 0, 0
    return 3, 1


def _fwd_t(s, Mp):
    """(form, topics per L2 group)"""
    n, K = s["n"], s["K"]
    if not s["split"]:
        return 1, 0
    NP = 2 if s["split"] == 2 else 3
    panel = 0.625 * 2.0 * NP * float(Mp) * Mp
    KG = max(1, min(K, int(2.0 * 1024 * 1024 / panel)))
    rtiles = cdiv(n, TILE)
    pairs = (rtiles + 1) // 2
    if s["split"] == 2:
        nct = cdiv(Mp, TILE)
        if Mp % 64 == 0 and 2 <= K <= 16 and pairs * nct > 32:
            KQ = K // 4 * 4
            KP = (K - KQ + 1) // 2
            return 4, (4 if KQ else 2 * min(KP, FWD_T_W1_KGP))
    return (2 if NP == 2 else 3), KG


def _a_k(s, Mp, cap):
    n, K, esz = s["n"], s["K"], s["esz"]
    nt, BR = cdiv(Mp, TILE), 128 // esz
    out = dict(ns=min(tn_nsplit(K, nt, n, BR, 2 if s["split"] else 3), cap), nst=0, ns1=0)
    if s["split"] == 2:
        out["nst"] = min(tn_topics_nsplit(K, Mp, n), cap)
        kgroups = cdiv(K, TNT_KT)
        if 10 * K >= 6 * kgroups * TNT_KT:
            ns1 = cap if cap < 64 else 64
            while ns1 > 8 and cdiv(n, ns1) < 8 * TN1_CH:
                ns1 -= 8
            if ns1 >= 8:
                ns1 &= ~7
            out["ns1"] = ns1
            return 4, kgroups, out
        return 3, kgroups, out
    return (2 if s["split"] else 1), 0, out


def _loc(s, Mp):
    K, esz = s["K"], s["esz"]
    if K <= LOC_KMAX and Mp % (16 * (16 // esz)) == 0 and K * Mp * esz <= 150 * KB:
        return 1
    return 3 if esz == 8 and K > 64 else 2


def _rows(s, Mp):
    """(form, 16-topic tiles, 16-word tiles); zeros where the thread form refuses the shape"""
    n, K, V, esz = s["n"], s["K"], s["V"], s["esz"]
    if s["rows_form"] == 1 or s["csr"]:
        return 3, 0, 0
    ldk = round_up(s["n_cap"], 4)
    nqpart = cdiv(Mp, 128 if s["ssz"] == 4 else 64)
    lim, grp = 1 << 32, 16 * esz
    fit = (max(K, nqpart) - 1) * ldk * esz + grp < lim and (K - 1) * n * esz + grp < lim
    if K <= 32 and V <= 64 and fit:
        return 1, (1 if K <= 16 else 2), (2 if V <= 32 else 4)
    kreg = K <= KMAX
    lds_for = lambda rb: 128 + (2 * K * V + rb * (K + 1) * (1 if kreg else 2) + rb * (V + 1)) * esz
    RB = 128
    while RB > 32 and lds_for(RB) > 150 * KB:
        RB >>= 1
    if lds_for(RB) > 150 * KB:
        return 0, 0, 0
    return 2, 0, 0


def _predict(s):
    """(form, 16-topic column blocks); zeros in mode 4 and where the route refuses the shape"""
    M, K, V, D, ts, mode = s["M"], s["K"], s["V"], s["D"], s["ssz"], s["predict_mode"]
    if mode == 4:
        return 0, 0
    if s["rows_form"] == 1 or (mode == 3 and s["csr"]):
        return (5, 0) if 128 + M * D * ts <= 150 * KB else (0, 0)
    M4, NB, DDt = round_up(M, 4), (1 if K <= 16 else 2), (2 if D <= 2 else DMAX)
    if K <= 32 and 128 + (M4 * DDt + K * V + 4 * 16 * (16 * NB + 1)) * ts <= 64 * KB:
        return 1, NB
    if K > KMAX:
        return (4, 0) if 128 + (M * D + K * V + 128 * (V + 1)) * ts <= 150 * KB else (0, 0)
    lds, in_lds = 128 + (M * D + K * V + K * M) * ts, True
    if lds > 64 * KB:
        in_lds, lds = False, lds - K * M * ts
    if lds > 150 * KB:
        return 0, 0
    return (2 if in_lds else 3), 0


def mm_plan(Mp, esz, batch, tiles, slab_bytes, beside_chain):
    """(form, slices, reduction indices per slice) of C = A B^T on `batch` M x M operands of esz-byte elements: 1 one launch, 2 the reduction
    of a SINGLE product in eight slices through the context's slab buffer - never for a product that runs beside the chain that uses it"""
    if beside_chain:
        return 1, 1, 0
    return mm_plan_old(Mp, esz, batch, tiles, slab_bytes)


def mm_plan_old(Mp, esz, batch, tiles, slab_bytes, beside_chain=False):
    """The rule before `beside_chain` was read: batch == 1 alone selects the split"""
    S = 8 if batch == 1 else 4
    kw = Mp // S
    BK = 32 if esz == 4 else 16
    if batch == 1 and slab_bytes and tiles * batch <= 256 and Mp >= 256 and Mp % S == 0 and kw % BK == 0 and S * batch * Mp * Mp * esz <= slab_bytes:
        return 2, S, kw
    return 1, 1, 0


def mm_tiles(Mp, esz):
    return cdiv(Mp, TILE) * cdiv(Mp, 128 if esz == 4 else 64)


def mm_forms(Mp, esz, ssz, K, unwhitened, plan=None):
    """(mm_chain, mm_sbar) of step_finish: the chain's single products in the solve precision on the main stream; Sbar_k = 2 A_k S_k, K products in
    the arrays' precision, beside the chain on the side stream in the whitened form and alone on the main stream in the unwhitened one.
    `plan`: the rule, mm_plan unless given."""
    plan = plan or mm_plan
    slab = 8 * Mp * Mp * ssz
    return plan(Mp, ssz, 1, mm_tiles(Mp, ssz), slab, False)[0], plan(Mp, esz, K, mm_tiles(Mp, esz), slab, not unwhitened)[0]


def forms(s):
    """The slots (by Engine.FORM_SLOTS' names, numbers) and the split counts EXTRA of a shape: a dict with the keys FIELDS."""
    n, K, esz = s["n"], s["K"], s["esz"]
    Mp = round_up(s["M"], MPAD)
    nt, BR = cdiv(Mp, TILE), 128 // esz
    cap = nsplit_cap(K, Mp, s["n_cap"], esz)
    out = {}
    out["wbar"], out["wbar_nslice"] = _wbar(s, Mp, cap)
    out["a_k"], out["a_k_kgroups"], ns = _a_k(s, Mp, cap)
    out.update(ns)
    out["fwd_t"], out["fwd_t_kg"] = _fwd_t(s, Mp)
    out["loc"] = _loc(s, Mp)
    out["ubar_q4"] = (K + 3) // 4 if K <= 16 else 4
    out["rows"], out["rows_kt"], out["rows_vt"] = _rows(s, Mp)
    out["gt"] = 2 if s["split"] else 1
    out["gt_ns"] = min(tn_nsplit_gt(K, nt, n, BR) if s["split"] else tn_nsplit(K, nt, n, BR, 3), cap)
    tn = esz == 4 and s["ssz"] == 8 and hyper_tn_on(s, Mp)
    out["hyper"] = 2 if tn else 1
    out["hyper_ns"] = min(tn_nsplit_gt(K, nt, n, BR), cap) if tn else 0
    out["predict"], out["predict_nb"] = _predict(s)
    out["mm_chain"], out["mm_sbar"] = mm_forms(Mp, esz, s["ssz"], K, s["unwhitened"])
    return out


def resolve(n, M, K, V, D=2, *, n_cap=None, dtype="f32", pure_fp32=False, store_t="auto", mfma_mode="auto", hyper_backward="auto",
            rows_form="auto", csr=False, learn_inducing=False, ard=False, kind="rbf", predict_mode=0, whiten=True):
    """Engine's keywords -> a shape, as Engine.__init__ and gdrf_ctx_create_ex resolve them: n_cap defaults to n, store_t "auto" is off,
    mfma_mode "auto" is f32 for float64 arrays or a stored T_k, bf16x6 for the all-fp32 arithmetic, f16x3 otherwise."""
    esz = 8 if dtype == "f64" else 4
    pure = bool(pure_fp32) and esz == 4
    ssz = 4 if pure else 8
    stored_t = store_t is True
    if mfma_mode == "auto":
        mfma_mode = "f32" if (esz != 4 or stored_t) else ("bf16x6" if pure else "f16x3")
    return dict(n=n, n_cap=n_cap or n, M=M, K=K, V=V, D=D, esz=esz, ssz=ssz, split={"f32": 0, "bf16x6": 1, "f16x3": 2}[mfma_mode],
                stored_t=int(stored_t), rows_form=int(rows_form == "streamed"), csr=int(csr), hyper_tn=int(hyper_backward == "tn"),
                learn_z=int(learn_inducing), ard=int(ard), per=0, kind=KINDS.index(kind), predict_mode=predict_mode, unwhitened=int(not whiten))


def line(s):
    """The shape as tests/host/forms_table.cpp reads it"""
    return " ".join(str(int(s[k])) for k in FIELDS)
