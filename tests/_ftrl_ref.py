"""Test-only reference for the FTRL-Proximal step (SPEC.md §4 "FTRL-Proximal"): the rule in NumPy float32, line for line as the SPEC writes it —
every line one fp32 operation rounded on its own, no fma — and the duplicate-key reduction of SPEC.md §4 (an fp64 sum per distinct key, rounded
once; a single occurrence is a copy).  NumPy's float32 add, multiply, divide and sqrt are correctly rounded and keep subnormals, so this is the
library's arithmetic exactly; `dtype=np.float64` runs the same lines in fp64 (the sanity checks of tests/test_ftrl.py)."""
import numpy as np

EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1


def ftrl_update(w, z, n, g, lr, beta, l1, l2, dtype=np.float32, fused=()):
    """One step on arrays of one shape -> (w', z', n').  The scalars are cast to `dtype` first.
    fused: which lines to compute the way a contracting compiler would, for the tests that show the reference can tell — "sw": z' = fma(-sig, w, z + g),
    "nn": n' = fma(g, g, n); both are emulated in fp64 and rounded once (exact for fp32 inputs up to the final rounding of the sum; dtype fp32 only)."""
    f = dtype
    w, z, n, g = (np.asarray(a, dtype=f) for a in (w, z, n, g))
    lr, beta, l1, l2 = f(lr), f(beta), f(l1), f(l2)
    with np.errstate(all="ignore"):
        gg = g * g
        nn = n + gg
        if "nn" in fused:
            nn = (n.astype(np.float64) + g.astype(np.float64) * g.astype(np.float64)).astype(f)
        sn = np.sqrt(nn)
        sig = (sn - np.sqrt(n)) / lr
        sw = sig * w
        zn = (z + g) - sw
        if "sw" in fused:
            zn = ((z + g).astype(np.float64) - sig.astype(np.float64) * w.astype(np.float64)).astype(f)
        den = (beta + sn) / lr + l2
        wn = np.where(np.abs(zn) <= l1, f(0.0), (np.copysign(l1, zn) - zn) / den).astype(f)   # a NaN z' fails the comparison and propagates
    return wn, zn, nn


def reduce_duplicates(keys, grads):
    """SPEC.md §4: -> (distinct keys, sorted; one fp32 gradient row per key = the fp64 sum of its occurrences' rows rounded once; a key that occurs once
    keeps its row bit for bit).  Reserved keys (EMPTY, RECLAIMED) are dropped."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    grads = np.asarray(grads, dtype=np.float32).reshape(keys.size, -1)
    live = keys > RECLAIMED_KEY
    keys, grads = keys[live], grads[live]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    if not ks.size:
        return ks, grads
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    counts = np.diff(np.concatenate([starts, [ks.size]]))
    with np.errstate(all="ignore"):
        summed = np.add.reduceat(grads[order].astype(np.float64), starts, axis=0).astype(np.float32)
    single = counts == 1
    summed[single] = grads[order][starts[single]]
    return ks[starts], summed


class FtrlRefTable:
    """A table of (key -> w, z, n) rows with the step of the library: absent keys ignored, duplicates reduced, one update per distinct key."""

    def __init__(self, dim, initial_accumulator=0.0):
        self.dim, self.init_acc = dim, np.float32(initial_accumulator)
        self.keys = np.empty(0, dtype=np.int64)
        self.w = self.z = self.n = np.empty((0, dim), dtype=np.float32)

    def insert(self, keys, rows):
        """new keys get z = +0.0, n = initial_accumulator; a key already stored gets the row only (insert's overwrite)"""
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        rows = np.asarray(rows, dtype=np.float32).reshape(keys.size, self.dim)
        old = dict(zip(self.keys.tolist(), range(self.keys.size)))
        new_k, new_r = [], []
        for k, r in zip(keys.tolist(), rows):
            if k in old:
                self.w[old[k]] = r
            else:
                old[k] = -1
                new_k.append(k); new_r.append(r)
        if new_k:
            m = len(new_k)
            self.keys = np.concatenate([self.keys, np.asarray(new_k, dtype=np.int64)])
            self.w = np.concatenate([self.w, np.asarray(new_r, dtype=np.float32).reshape(m, self.dim)])
            self.z = np.concatenate([self.z, np.zeros((m, self.dim), dtype=np.float32)])
            self.n = np.concatenate([self.n, np.full((m, self.dim), self.init_acc, dtype=np.float32)])
            order = np.argsort(self.keys)
            self.keys, self.w, self.z, self.n = self.keys[order], self.w[order], self.z[order], self.n[order]

    def set_state(self, keys, z, n):
        i = self._index(np.asarray(keys, dtype=np.int64))
        self.z[i], self.n[i] = np.asarray(z, dtype=np.float32), np.asarray(n, dtype=np.float32)

    def _index(self, keys):
        i = np.searchsorted(self.keys, keys)
        assert np.array_equal(self.keys[np.minimum(i, self.keys.size - 1)], keys), "a key is not stored"
        return i

    def apply(self, keys, grads, lr, beta=1.0, l1=0.0, l2=0.0, grad_index=None, fused=()):
        grads = np.asarray(grads, dtype=np.float32)
        if grad_index is not None:
            grads = grads.reshape(-1, self.dim)[np.asarray(grad_index, dtype=np.int64)]
        uk, ug = reduce_duplicates(keys, grads)
        i = np.searchsorted(self.keys, uk)
        held = (i < self.keys.size) & (self.keys[np.minimum(i, max(self.keys.size - 1, 0))] == uk) if self.keys.size else np.zeros(uk.size, dtype=bool)
        i, ug = i[held], ug[held]
        self.w[i], self.z[i], self.n[i] = ftrl_update(self.w[i], self.z[i], self.n[i], ug, lr, beta, l1, l2, fused=fused)

    def export_sorted(self):
        """[keys, w, z, n] sorted by key: what tests/_apply_cases.export_sorted gives for a table"""
        return [self.keys.copy(), self.w.copy(), self.z.copy(), self.n.copy()]
