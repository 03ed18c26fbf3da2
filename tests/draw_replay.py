"""A host restatement of the token draws (test infrastructure, CPU only): Philox4x32-10, the 24-bit uniform, the candidate order and
the inverse CDF, in Python integers and float64, vectorised over rows.  It predicts the id of every single draw of
rwkv7_sample_rows_f32 / _tail_f32, rwkv7_sample_slots_f32, the XY slot draw and the RAS entries from the contract in
include/rwkv7_hip.h and the layout notes of csrc/sampling_common.h; nothing here is imported from the kernels' side.

What is exact.  The counter and key words, the uniform u = (word >> 8) / 2^24, x = float32(logit) * float32(1 / temperature), the
allowed range, the suppressed ids, the min-EOS bar, the argmax, the candidate list (value descending, index ascending, ties at the
k-th value, 128 at most) and d_j = float32(x_j - x_0): integers and single IEEE operations the host reproduces bit for bit.

What is not.  The kernel forms exp(d_j) with __expf and adds in fp32; the replay uses float64.  A prediction is therefore marked
AMBIGUOUS when a comparison the kernel makes could go the other way within a margin eps * mass, and comes with the ADMISSIBLE set of
ids it could flip to.  eps is a bound derived here, per row, from the kernel's arithmetic (u = 2^-24, the unit roundoff of fp32):

  * __expf(d) is exp2(fl(d * fl(log2 e))) with a 1-ulp hardware exp2: the argument carries a relative error of 1.5 u (constant and
    product), which the exponential turns into 1.5 |d| u, plus 2 u for the 1-ulp result: (2 + 1.5 |d|) u per term.  Terms below
    2^-126 flush to zero on the device; their absolute size is far under any margin.  In the whole-row draw x_j - mx may be
    contracted with the temperature product into one fma, which moves d_j by at most (|x_j| + |d_j|) u: (2 + 2.5 |d| + |x|) u there.
    A prefix of the CDF inherits the MASS-WEIGHTED mean of these, E = sum_j r_j e_j / sum_j e_j, relative to the total mass: the
    replay evaluates E on the row itself instead of taking the largest |d| (which the few terms that far down do not deserve: at
    |d| = 88, the flush threshold, it would be 134 u).
  * sums: a thread adds its EPT elements one after the other (EPT = 5 / 33 / 60 for ranges up to 1280 / 8448 / 15360 ids), the 256
    thread sums go through a 6-step scan inside the waves and up to 3 wave offsets.  Whole-row draw: the target u * total has depth
    (EPT - 1) + 9 + 1, the running sum the owner compares with it (EPT - 1) + 9 + 1 (incl - s) + EPT: 3 EPT + 20 in all.
    Candidates (one per thread, 128 at most): the scan alone on either side, 2 * 9, plus the product with top_p or u and cj - ej: 22.
    RAS nucleus: p_j = __expf / z with z a butterfly sum of depth EPT + 7 and one division: 2 (EPT + 18) + 4.

      eps_full(row) = (3 EPT + 20 + 2 E) u      eps_cand(row) = (22 + 2 E) u      eps_ras(row) = (2 EPT + 40 + 2 E) u

    For the Gaussian rows of the tests E is 5 .. 25, so eps is 2^-19 for the candidates and 2^-16 for the widest whole-row draw:
    both below the 2^-15 of the first CPU trial.  The bound is worst case and linear; it was not tuned against any result.

A draw is ambiguous if a CDF step lies within eps * mass of its target, or a strictly-higher mass within eps * z of the top-p cut
-- unless every cut and target inside the margin still gives the predicted id (a rank of negligible mass at the cut, far from the
target), in which case the prediction stands and is compared exactly.  The admissible set holds every id whose CDF interval
meets [target - eps * mass, target + eps * mass] under every cut the margin allows.  The whole-row draw adds the row's argmax (the kernel's answer when rounding leaves no thread owning the target) and, when
the target is within the margin of the total, everything from there to the end of the kernel's element order.

`twin_*`: the same chain in numpy float32 in the kernel's order of operations (thread sums, wave scans, wave offsets).  It is no
reference, only evidence that fp32 arithmetic in that order stays inside the margin (tests/test_draw_replay.py); its `alter` argument
builds deliberately wrong variants to show that a comparison against the replay notices them."""
import numpy as np
import torch

M32 = 0xFFFFFFFF
THREADS, MAX_CAND = 256, 128
CTR_ROWS, CTR_RAS = 0x5A17, 0x7A5
U = 2.0 ** -24
CAP = 0.03           # the largest share of ambiguous draws a test case may have
F32 = np.float32
NEG = F32(-np.inf)


# ------------------------------------------------------------------------------------------------------------------- generator
def philox4x32_10(counter4, key2):
    """Philox4x32-10 (Salmon et al. 2011, Random123): four 32-bit counter words and two key words (ints or arrays that broadcast)
    -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in counter4]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in key2]
    m0, m1, w0, w1, s32, m = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 32, M32))
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                        # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m, (p0 >> s32) ^ c[3] ^ k[1], p0 & m]
        k = [(k[0] + w0) & m, (k[1] + w1) & m]
    return tuple(c)


def u01(word):
    """the top 24 bits of a word as a number in [0, 1): exact in float32 and float64 alike"""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


def split64(v):
    """low and high 32-bit words of 64-bit integers of either sign (Python ints: no overflow)"""
    flat = [int(t) for t in np.asarray(v, dtype=object).reshape(-1)]
    shape = np.shape(v)
    lo = np.array([t & M32 for t in flat], dtype=np.uint64).reshape(shape)
    hi = np.array([(t >> 32) & M32 for t in flat], dtype=np.uint64).reshape(shape)
    return lo, hi


def draw_words(seed, step, word2, word3):
    """the four output words of the draw's counter (lo32(step), hi32(step), word2, word3) under the key (lo32(seed), hi32(seed))"""
    slo, shi = split64(step)
    klo, khi = split64(seed)
    return philox4x32_10((slo, shi, word2, word3), (klo, khi))


def ept_class(max_domain):
    """elements per thread of the kernel instance that serves a launch whose largest allowed range has max_domain ids"""
    return 5 if max_domain <= 5 * THREADS else 33 if max_domain <= 33 * THREADS else 60


def kernel_order(m):
    """the element order of the whole-row CDF: thread t = j % 256 major, then j // 256"""
    j = np.arange(m)
    return np.lexsort((j // THREADS, j % THREADS))


# ----------------------------------------------------------------------------------------------------------------------- rows
def scaled_rows(logits, col0, lo, hi, inv_temp, dropped=(), bar=None):
    """x [R, hi - lo] float32 = float32(logit) * float32(inv_temp) over the allowed range [lo, hi) of a segment whose id 0 sits in
    column col0; -inf at the `dropped` ids (segment-relative) and, in the rows where `bar` = (id, bool [R]) says so, at that id"""
    lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    assert lg.dtype == np.float32
    x = lg[:, col0 + lo:col0 + hi] * np.asarray(inv_temp, dtype=F32).reshape(-1, 1)
    assert x.dtype == np.float32
    x = np.array(x, dtype=F32)
    for t in dropped:
        if lo <= t < hi:
            x[:, t - lo] = NEG
    if bar is not None and lo <= bar[0] < hi:
        x[np.asarray(bar[1], dtype=bool), bar[0] - lo] = NEG
    return x


def inv_temperature(temperature, do_sample=True):
    """1.f / temperature as the launcher forms it (1 for argmax)"""
    return F32(1.0) / F32(temperature) if do_sample else F32(1.0)


def candidates(x, want, ties):
    """The `want` largest of every row by (value descending, index ascending), -inf never; with `ties` every further element equal
    to the last one as well; 128 at most, the smaller indices first.  -> values [R, K] float32 (-inf beyond n), indices [R, K], n [R]"""
    R, m = x.shape
    want, K = min(want, m), min(MAX_CAND, m)
    xt = torch.from_numpy(x)
    kth = torch.topk(xt, want, dim=1).values[:, -1:]                 # -inf: fewer ids than wanted have a finite value
    mask = (xt >= kth) & (xt > float("-inf"))
    cnt = mask.sum(1)
    v, i = torch.topk(torch.where(mask, xt, torch.full_like(xt, float("-inf"))), K, dim=1)
    o = torch.argsort(i, dim=1, stable=True)
    v, i = v.gather(1, o), i.gather(1, o)
    o = torch.argsort(-v, dim=1, stable=True)
    v, i = v.gather(1, o).numpy().copy(), i.gather(1, o).numpy().copy()
    for r in torch.nonzero(cnt > K).flatten().tolist():              # more ties than the list holds: which 128 matters
        idx = np.flatnonzero(mask[r].numpy())
        idx = idx[np.lexsort((idx, -x[r, idx].astype(np.float64)))][:K]
        v[r], i[r] = x[r, idx], idx
    n = np.minimum(cnt.numpy(), K if ties else want)
    v[np.arange(K)[None, :] >= n[:, None]] = NEG
    return v, i, n


class Draws:
    """what a replay returns: pred (the predicted ids), amb (bool, same shape) and adm {index tuple: frozenset of admissible ids}
    for the ambiguous draws (an unambiguous draw admits its prediction alone)"""

    def __init__(self, pred, amb, adm):
        self.pred, self.amb, self.adm = np.asarray(pred, dtype=np.int64), np.asarray(amb, dtype=bool), adm

    def admissible(self, idx):
        idx = tuple(int(t) for t in np.atleast_1d(idx))
        return self.adm[idx] if self.amb[idx] else frozenset([int(self.pred[idx])])

    def share(self):
        return float(self.amb.mean()) if self.amb.size else 0.0

    def compare(self, ids):
        """-> (mismatches among the unambiguous draws, ambiguous draws whose id is not admissible)"""
        ids = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        ids = ids.reshape(self.pred.shape)
        wrong = int(((ids != self.pred) & ~self.amb).sum())
        out = sum(int(ids[idx]) not in self.adm[idx] for idx in zip(*np.nonzero(self.amb)))
        return wrong, out

    def offset(self, add):
        return Draws(self.pred + add, self.amb, {k: frozenset(t + int(add) for t in v) for k, v in self.adm.items()})


def _topk_one(e, C, n, tp, u, eps, nk):
    """ranks whose CDF interval meets the margin when the first nk ranks are kept (one row)"""
    kept = C[nk - 1]
    t, dl = u * kept, eps * kept
    lo = min(int((C[:nk] <= t - dl).sum()), nk - 1)
    hi = min(int((C[:nk] <= t + dl).sum()), nk - 1)
    return range(lo, hi + 1)


class TopK:
    """temperature -> top-k (ties at the k-th value stay) -> top-p -> inverse CDF over the candidate order, for the rows of x.
    ras = (z64 [R], mx [R]): the RAS nucleus instead: p_j = exp(v_j - mx) / z, kept while the mass before is < top_p (rank 0 is
    not special), no tie extension, `zero` = id whose weight is removed after the cut (EOS while it is rejected; -1: none)."""

    def __init__(self, x, top_k, top_p, ties=True, ras=None, zero=-1, ept=60):
        self.cv, self.ci, self.n = candidates(x, top_k, ties)
        R, K = self.cv.shape
        self.R, self.K, self.ras = R, K, ras is not None
        self.tp = np.broadcast_to(np.asarray(top_p, dtype=F32).astype(np.float64), (R,))
        valid = np.arange(K)[None, :] < self.n[:, None]
        ref = self.cv[:, :1] if ras is None else ras[1].reshape(-1, 1).astype(F32)
        with np.errstate(invalid="ignore"):
            d = np.where(valid, (self.cv - ref).astype(F32), F32(0)).astype(np.float64)
        e = np.where(valid, np.exp(d), 0.0)
        if ras is not None:
            e = e / ras[0].reshape(-1, 1)
        C = np.cumsum(e, 1)
        z = C[:, -1] if ras is None else np.ones(R)
        S = C - e                                                     # strictly-higher mass
        E = np.where(self.n > 0, ((2 + 1.5 * np.abs(d)) * e).sum(1) / np.maximum(C[:, -1], 1e-300), 2.0)
        self.eps = U * ((22 if ras is None else 2 * ept + 40) + 2 * E)
        rank = np.arange(K)[None, :]
        cut = (self.tp * z)[:, None]
        mz = (self.eps * z)[:, None]
        first = (rank == 0) if ras is None else np.zeros((1, K), dtype=bool)
        self.keep = valid & (first | (S < cut))
        self.cut_amb = (valid & ~first & (np.abs(S - cut) <= mz)).any(1)
        self.nk_lo = (valid & (first | (S < cut - mz))).sum(1)
        self.nk_hi = (valid & (first | (S < cut + mz))).sum(1)
        self.nk = self.keep.sum(1)
        if ras is not None:                                           # the weight of the rejected id goes after the cut
            e = np.where(self.ci == zero, 0.0, e)
            C = np.cumsum(e, 1)
        self.e, self.C = e, C

    def draw(self, u):
        """u [R] -> Draws over the RANGE-relative ids (no candidate: id 0, or -1 for the RAS nucleus whose kept mass is 0)"""
        R, ar = self.R, np.arange(self.R)
        nk1 = np.maximum(self.nk, 1) - 1
        kept = self.C[ar, nk1]
        t, dl = u * kept, self.eps * kept
        inside = np.arange(self.K)[None, :] < self.nk[:, None]
        pos = self.e > 0 if self.ras else np.ones_like(inside)
        # first kept rank whose inclusive mass exceeds the target; the last kept rank (with weight) catches overshoot
        last = np.where((inside & pos).any(1), self.K - 1 - np.argmax((inside & pos)[:, ::-1], 1), 0)
        pick = np.minimum(((self.C <= t[:, None]) & inside).sum(1), last)
        lo = np.minimum(((self.C <= (t - dl)[:, None]) & inside).sum(1), last)
        hi = np.minimum(((self.C <= (t + dl)[:, None]) & inside).sum(1), last)
        none = (self.nk == 0) | (kept <= 0)
        pred = np.where(none, -1 if self.ras else 0, self.ci[ar, pick])
        amb = ((lo != hi) | self.cut_amb) & (self.n > 0)
        if self.ras:
            amb &= ~(none & ~self.cut_amb)
        adm = {}
        for r in np.flatnonzero(amb):
            ids = set()
            for nk in range(max(int(self.nk_lo[r]), 1), max(int(self.nk_hi[r]), 1) + 1):
                if self.ras:
                    C = np.cumsum(np.where(np.arange(self.K) < nk, self.e[r], 0.0))
                    if C[-1] <= 0:
                        ids.add(-1)
                        continue
                    w = np.flatnonzero((np.arange(self.K) < nk) & (self.e[r] > 0))
                    tt, dd = u[r] * C[-1], self.eps[r] * C[-1]
                    a = min(int((C <= tt - dd).sum()), w[-1])
                    b = min(int((C <= tt + dd).sum()), w[-1])
                    ids.update(int(self.ci[r, j]) for j in w if a <= j <= b)
                else:
                    ids.update(int(self.ci[r, j]) for j in _topk_one(self.e[r], self.C[r], self.n[r], self.tp[r], u[r], self.eps[r], nk))
            if ids == {int(pred[r])}:                                 # every cut and target inside the margin gives the same id
                amb[r] = False
            else:
                adm[(int(r),)] = frozenset(ids)
        return Draws(pred, amb, adm)


class Full:
    """the inverse CDF over a whole row in the kernel's element order, weights exp(x_j - max) (without `skip`, -1: none)"""

    def __init__(self, x, ept, skip=-1):
        R, m = x.shape
        self.R, self.m, self.order = R, m, kernel_order(m)
        self.mx = x.max(1)
        self.arg = np.argmax(x, 1)                                    # first maximum
        with np.errstate(invalid="ignore"):
            d = (x - self.mx[:, None]).astype(F32).astype(np.float64)
        w = np.where(np.isfinite(d), np.exp(d), 0.0)
        if skip >= 0:
            w[:, skip] = 0.0
        r = np.where(w > 0, (2 + 2.5 * np.abs(np.where(w > 0, d, 0.0)) + np.abs(np.where(w > 0, x, F32(0)))) * w, 0.0)
        self.z = w.sum(1)                                             # (RAS: the softmax denominator is taken with `skip` = -1)
        self.C = np.cumsum(w[:, self.order], 1)
        self.total = self.C[:, -1]
        E = r.sum(1) / np.maximum(w.sum(1), 1e-300)
        self.E = E
        self.eps = U * (3 * ept + 20 + 2 * E)
        wo = w[:, self.order] > 0
        self.pos = wo
        self.last = np.where(wo.any(1), m - 1 - np.argmax(wo[:, ::-1], 1), -1)

    def draw(self, u):
        """u [R] -> Draws over range-relative ids (a row without weight: the first maximum)"""
        t, dl = u * self.total, self.eps * self.total
        cnt = lambda v: (self.C <= v[:, None]).sum(1)
        pick, lo, hi = cnt(t), cnt(t - dl), cnt(t + dl)
        none = self.last < 0
        over = (hi > self.last) & ~none
        pick, lo, hi = (np.minimum(v, np.maximum(self.last, 0)) for v in (pick, lo, hi))
        pred = np.where(none, self.arg, self.order[pick])
        amb = ((lo != hi) | over) & ~none
        adm = {}
        for r in np.flatnonzero(amb):
            b = self.last[r] if over[r] else hi[r]
            js = np.arange(lo[r], b + 1)
            adm[(int(r),)] = frozenset(self.order[js[self.pos[r, js]]].tolist()) | {int(self.arg[r])}
        return Draws(pred, amb, adm)


class Greedy:
    def __init__(self, x):
        self.arg = np.argmax(x, 1)                                    # the first maximum; a row of -inf: id 0

    def draw(self, u):
        return Draws(self.arg, np.zeros(self.arg.shape, dtype=bool), {})


def row_law(x, do_sample, top_k, top_p, ept):
    """the u -> id map of every row of x"""
    if not do_sample:
        return Greedy(x)
    return TopK(x, top_k, top_p) if top_k > 0 else Full(x, ept)


def replay_rows(logits, seg_len, launches, seg_off=None, allow=None, suppress=None, do_sample=False, top_k=0, top_p=1.0, temperature=1.0,
                min_eos=None, inv_temp=None, word2=None):
    """rwkv7_sample_rows_f32 / _tail_f32 (the raw draws) for every (seed, step) of `launches` -> [Draws with arrays [R, nseg]].
    inv_temp: the factor itself instead of 1 / temperature (the per-slot entries store it); word2 [R, nseg]: the counter's third
    word instead of row * nseg + seg (the per-slot entries: 0, the XY slot draw: the channel)."""
    R, nseg = logits.shape[0], len(seg_len)
    if seg_off is None:
        seg_off = np.concatenate([[0], np.cumsum(seg_len)[:-1]]).tolist()
    dom = [(0, int(n)) if allow is None else (max(int(allow[s][0]), 0), min(int(allow[s][1]), int(n))) for s, n in enumerate(seg_len)]
    ept = ept_class(max(hi - lo for lo, hi in dom))
    it = inv_temperature(temperature, do_sample) if inv_temp is None else F32(inv_temp)
    if word2 is None:
        word2 = np.arange(R * nseg, dtype=np.uint64).reshape(R, nseg)
    laws, out = {}, []
    for seed, step in launches:
        barred = min_eos is not None and min_eos[0] >= 0 and step < min_eos[1]
        pred, amb, adm = np.zeros((R, nseg), dtype=np.int64), np.zeros((R, nseg), dtype=bool), {}
        u = u01(draw_words(seed, step, word2, CTR_ROWS)[0])
        for s, (lo, hi) in enumerate(dom):
            if (s, barred) not in laws:
                x = scaled_rows(logits, seg_off[s], lo, hi, it, suppress or (), (min_eos[0], np.full(R, True)) if barred else None)
                laws[(s, barred)] = row_law(x, do_sample, top_k, top_p, ept)
            d = laws[(s, barred)].draw(u[:, s]).offset(lo)
            pred[:, s], amb[:, s] = d.pred, d.amb
            adm.update({(k[0], s): v for k, v in d.adm.items()})
        out.append(Draws(pred, amb, adm))
    return out


def replay_tail(draws, steps, eos, pad, seq_ld, fill=-7):
    """What the decode loop's tail keeps over consecutive launches whose raw draws are `draws` (predicted or observed ids [R] per
    step): finished rows emit pad, EOS ends a row, the id goes to column `step`.  -> kept ids per step, unfinished per step, seq"""
    R = len(draws[0])
    unf, seq = np.ones(R, dtype=bool), np.full((R, seq_ld), fill, dtype=np.int64)
    kept, unfs = [], []
    for ids, step in zip(draws, steps):
        ids = np.where(unf, np.asarray(ids, dtype=np.int64), pad)
        unf = unf & (ids != eos)
        if step < seq_ld:
            seq[:, step] = ids
        kept.append(ids)
        unfs.append(unf.copy())
    return kept, unfs, seq


# ------------------------------------------------------------------------------------------------------------------------ RAS
class RasRow:
    """everything about one logits row that the steps of rwkv7_ras_step_f32 share"""

    def __init__(self, logits, eos, top_p, top_k):
        lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
        self.x = np.array(lg, dtype=F32).reshape(1, -1)
        self.V, self.eos, self.top_p, self.top_k = self.x.shape[1], int(eos), top_p, int(top_k)
        self.ept = ept_class(self.V)
        self._full, self._nuc = {}, {}

    def full(self, ignore):
        if ignore not in self._full:
            self._full[ignore] = Full(self.x, self.ept, self.eos if ignore else -1)
        return self._full[ignore]

    def nucleus(self, ignore):
        if ignore not in self._nuc:
            f = self.full(False)
            self._nuc[ignore] = TopK(self.x, min(self.top_k, self.V), self.top_p, ties=False, ras=(f.z, f.mx),
                                     zero=self.eos if ignore else -1, ept=self.ept)
        return self._nuc[ignore]


def replay_ras(row, seed, step, ring, n_ignore, win_size, tau_r):
    """One step of rwkv7_ras_step_f32 on a RasRow with the ring as it stands -> (id, ambiguous, admissible ids)"""
    ignore = step < n_ignore
    wx, wy, wz, _ = draw_words(seed, step, 0, CTR_RAS)
    full = row.full(ignore).draw(u01(wx).reshape(1))
    alt = row.full(ignore).draw(u01(wy).reshape(1))
    nuc = row.nucleus(ignore).draw(u01(wz).reshape(1))
    ring = [int(t) for t in ring]
    thr = F32(win_size) * F32(tau_r)

    def outcome(c):
        """candidate c (-1: the kept set holds nothing but EOS) -> the ids the step can emit, first the predicted one"""
        src = [alt] if c < 0 else []
        cands = [(int(alt.pred[0]), alt.admissible(0))] if c < 0 else [(c, frozenset([c]))]
        ids, amb = [], False
        for p, adm_c in cands:
            for cc in [p] + sorted(adm_c - {p}):
                if F32(ring.count(cc)) >= thr:
                    ids += [int(full.pred[0])] + sorted(full.admissible(0) - {int(full.pred[0])})
                    amb |= bool(full.amb[0])
                else:
                    ids.append(cc)
        return ids, amb or any(bool(s.amb[0]) for s in src)

    ids, amb = outcome(int(nuc.pred[0]))
    pred = ids[0]
    adm = set(ids)
    if nuc.amb[0]:
        amb = True
        for c in nuc.admissible(0):
            adm.update(outcome(c)[0])
    return pred, bool(amb), frozenset(adm)


def ras_bookkeeping(tok, ring, ptr, step, eos, win_size):
    """the loop's bookkeeping after a step: an emitted id goes into the ring at ptr, EOS is not appended, the step index moves on"""
    ring = list(ring)
    if tok != eos:
        ring[ptr] = tok
        ptr = (ptr + 1) % win_size
    return ring, ptr, step + 1


def replay_ras_sequence(row, seed, ring, ptr, n_steps, n_ignore, win_size, tau_r, observed=None, step0=0):
    """Consecutive steps, the ring carried on the host.  observed: the ids a device run emitted; after an ambiguous step the host
    goes on from the observed id if it is admissible (so the comparison stays exact for the rest of the sequence).
    -> [(pred, ambiguous, admissible, ring after, ptr after, step after)]"""
    ring, out, step = [int(t) for t in ring], [], step0
    for i in range(n_steps):
        pred, amb, adm = replay_ras(row, seed, step, ring, n_ignore, win_size, tau_r)
        tok = pred
        if observed is not None and amb and int(observed[i]) in adm:
            tok = int(observed[i])
        ring, ptr, step = ras_bookkeeping(tok, ring, ptr, step, row.eos, win_size)
        out.append((pred, amb, adm, list(ring), ptr, step))
    return out


# ------------------------------------------------------------------------------------------------------------- the fp32 twin
def _scan32(v):
    """inclusive prefix sum over 256 lanes as the kernel forms it: six shift-and-add steps inside each wave of 64, then the
    earlier waves' totals one after the other -> (prefix [R, 256], total [R]), float32 throughout"""
    R = v.shape[0]
    v = np.array(v, dtype=F32).reshape(R, 4, 64)
    for d in (1, 2, 4, 8, 16, 32):
        t = np.zeros_like(v)
        t[:, :, d:] = v[:, :, :-d]
        v = v + t
    w = v[:, :, 63]
    total = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    out = v.copy()
    out[:, 1] = v[:, 1] + w[:, 0:1]
    out[:, 2] = (v[:, 2] + w[:, 0:1]) + w[:, 1:2]
    out[:, 3] = ((v[:, 3] + w[:, 0:1]) + w[:, 1:2]) + w[:, 2:3]
    return out.reshape(R, 256), total


def _sum32(v):
    """block sum: butterfly inside each wave, then (w0 + w1) + (w2 + w3)"""
    R = v.shape[0]
    v = np.array(v, dtype=F32).reshape(R, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    return (v[:, 0, 0] + v[:, 1, 0]) + (v[:, 2, 0] + v[:, 3, 0])


def _lanes(a, fill):
    out = np.full((a.shape[0], THREADS), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def twin_topk(x, top_k, top_p, u, alter=()):
    """fp32 twin of the candidate draw.  alter: "cut_le" (the top-p cut with <= instead of <), "no_ties" (ties at the k-th value
    dropped) -> range-relative ids [R]"""
    cv, ci, n = candidates(x, top_k, "no_ties" not in alter)
    R = x.shape[0]
    cvl, cil = _lanes(cv, NEG), _lanes(ci, 0)
    lane = np.arange(THREADS)[None, :]
    valid = lane < n[:, None]
    with np.errstate(invalid="ignore"):
        e = np.where(valid, np.exp((cvl - cvl[:, :1]).astype(F32)), F32(0)).astype(F32)
    cj, z = _scan32(e)
    lim = (F32(top_p) * z)[:, None].astype(F32)
    below = (cj - e <= lim) if "cut_le" in alter else (cj - e < lim)
    keep = valid & ((lane == 0) | below)
    _, kept = _scan32(np.where(keep, e, F32(0)))
    target = (u.astype(F32) * kept).astype(F32)
    pick = (keep & (cj <= target[:, None])).sum(1)
    nk = keep.sum(1)
    return np.where(nk > 0, cil[np.arange(R), np.minimum(pick, np.maximum(nk, 1) - 1)], 0)


def twin_full(x, u, ept, skip=-1, alter=()):
    """fp32 twin of the whole-row draw: per-thread sums over elements t + 256 e, the scan, the owner's walk.  alter:
    "index_order" (thread t owns the ept consecutive elements from t * ept: the CDF in plain index order) -> ids [R], -1 -> argmax"""
    R, m = x.shape
    xp = np.full((R, ept * THREADS), NEG, dtype=F32)
    xp[:, :m] = x
    e_, t_ = np.meshgrid(np.arange(ept), np.arange(THREADS), indexing="ij")
    jmap = (t_ * ept + e_) if "index_order" in alter else (t_ + THREADS * e_)       # [ept, 256] element of (e, thread)
    mx = x.max(1)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((xp[:, jmap] - mx[:, None, None]).astype(F32)).astype(F32)       # [R, ept, 256]
        if skip >= 0:
            w = np.where(jmap[None] == skip, F32(0), w)
        s = np.zeros((R, THREADS), dtype=F32)
        for e in range(ept):
            s = s + w[:, e]
        incl, total = _scan32(s)
        before = incl - s
        target = (u.astype(F32) * total).astype(F32)[:, None]
        qual = (s > 0) & (target >= before) & ((target < incl) | (incl >= total[:, None]))
        c, last, done = before.copy(), np.full((R, THREADS), -1), np.zeros((R, THREADS), dtype=bool)
        for e in range(ept):
            act = ~done & (w[:, e] > 0)
            last = np.where(act, jmap[e][None, :], last)
            c = np.where(act, c + w[:, e], c).astype(F32)
            done |= act & (c > target)
    pick = np.where(qual, last, -1).max(1)
    return np.where(pick >= 0, pick, np.argmax(x, 1))


def twin_rows(logits, seg_len, launches, seg_off=None, allow=None, suppress=None, do_sample=False, top_k=0, top_p=1.0, temperature=1.0,
              min_eos=None, alter=()):
    """fp32 twin of replay_rows -> [ids [R, nseg]].  alter: twin_topk's and twin_full's, "no_word2" (the workgroup index left out
    of the counter), "no_seed_hi" (the upper half of the seed left out of the key)"""
    R, nseg = logits.shape[0], len(seg_len)
    if seg_off is None:
        seg_off = np.concatenate([[0], np.cumsum(seg_len)[:-1]]).tolist()
    dom = [(0, int(n)) if allow is None else (max(int(allow[s][0]), 0), min(int(allow[s][1]), int(n))) for s, n in enumerate(seg_len)]
    ept = ept_class(max(hi - lo for lo, hi in dom))
    it = inv_temperature(temperature, do_sample)
    word2 = np.arange(R * nseg, dtype=np.uint64).reshape(R, nseg) * np.uint64("no_word2" not in alter)
    out, xs = [], {}
    for seed, step in launches:
        barred = min_eos is not None and min_eos[0] >= 0 and step < min_eos[1]
        u = u01(draw_words(seed & M32 if "no_seed_hi" in alter else seed, step, word2, CTR_ROWS)[0])
        ids = np.zeros((R, nseg), dtype=np.int64)
        for s, (lo, hi) in enumerate(dom):
            if (s, barred) not in xs:
                xs[(s, barred)] = scaled_rows(logits, seg_off[s], lo, hi, it, suppress or (), (min_eos[0], np.full(R, True)) if barred else None)
            x = xs[(s, barred)]
            if not do_sample:
                ids[:, s] = lo + np.argmax(x, 1)
            elif top_k > 0:
                ids[:, s] = lo + twin_topk(x, top_k, top_p, u[:, s], alter)
            else:
                ids[:, s] = lo + twin_full(x, u[:, s], ept, -1, alter)
        out.append(ids)
    return out


def twin_ras(row, seed, step, ring, n_ignore, win_size, tau_r):
    """fp32 twin of one rwkv7_ras_step_f32 step on a RasRow -> id"""
    x, eos, ept = row.x, row.eos, row.ept
    ignore = step < n_ignore
    wx, wy, wz, _ = draw_words(seed, step, 0, CTR_RAS)
    skip = eos if ignore else -1
    full = int(twin_full(x, u01(wx).reshape(1), ept, skip)[0])
    alt = int(twin_full(x, u01(wy).reshape(1), ept, skip)[0])
    mx = x.max(1)
    xp = np.full((1, ept * THREADS), NEG, dtype=F32)
    xp[:, :row.V] = x
    zs = np.zeros((1, THREADS), dtype=F32)
    for e in range(ept):
        zs = zs + np.exp((xp[:, e * THREADS:(e + 1) * THREADS] - mx[:, None]).astype(F32)).astype(F32)
    z = _sum32(zs)
    cv, ci, n = candidates(x, min(row.top_k, row.V), False)
    cvl, cil = _lanes(cv, NEG), _lanes(ci, 0)
    lane = np.arange(THREADS)[None, :]
    valid = lane < n[:, None]
    pj = np.where(valid, np.exp((cvl - mx[:, None]).astype(F32)).astype(F32) / z[:, None], F32(0)).astype(F32)
    cj, _ = _scan32(pj)
    keep = valid & (cj - pj < F32(row.top_p))
    wj = np.where(keep & ~(ignore & (cil == eos)), pj, F32(0)).astype(F32)
    mj, mass = _scan32(wj)
    target = (u01(wz).astype(F32) * mass).astype(F32)
    cand = alt
    if mass[0] > 0:
        first = np.flatnonzero((wj[0] > 0) & (mj[0] > target[0]))
        lastw = np.flatnonzero(wj[0] > 0)
        cand = int(cil[0, first[0] if first.size else lastw[-1]])
    rep = [int(t) for t in ring].count(cand)
    return full if F32(rep) >= F32(win_size) * F32(tau_r) else cand


def interval_law(law, r, n_ids):
    """total length of the u-interval of every id for row r of a TopK / Full law: the probability the replay gives each id"""
    p = np.zeros(n_ids)
    if isinstance(law, Full):
        w = np.diff(np.concatenate([[0.0], law.C[r]])) / law.total[r]
        p[law.order] = w
    else:
        nk = int(law.nk[r])
        e = np.where(np.arange(law.K) < nk, law.e[r], 0.0)
        np.add.at(p, law.ci[r, :law.K], e / e.sum())
    return p
