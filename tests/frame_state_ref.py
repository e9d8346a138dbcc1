"""Float64 restatement of the five frame-state operations (csrc/frame_state.hip) in plain numpy / Python:
what the kernels are held to where the fixture of the reference's own Embedding (tests/golden/frame_state_cases.npz) does not
reach."""
import numpy as np


def clamp_rows(idx, n):
    return np.clip(np.asarray(idx, np.int64).reshape(-1), 0, n - 1)


def code_lookup_fwd(table, idx, max_norm):
    """-> (table after the in-place renorm, out (B,D)); float64.  The decision `norm > max_norm` and the scale
    max_norm / (norm + 1e-7) are torch's embedding_renorm_; max_norm None or <= 0: no renorm."""
    t = np.array(table, np.float64)
    rows = clamp_rows(idx, t.shape[0])
    if max_norm is not None and max_norm > 0:
        for r in sorted(set(rows.tolist())):
            norm = np.sqrt((t[r] * t[r]).sum())
            if norm > max_norm:
                t[r] *= max_norm / (norm + 1e-7)
    return t, t[rows]


def code_lookup_bwd(dout, idx, n):
    """-> the dense (N,D) gradient: row r = the sum of dout[b] over idx[b] = r, in increasing b; zeros elsewhere"""
    g = np.asarray(dout, np.float64)
    rows = clamp_rows(idx, n)
    out = np.zeros((n, g.shape[1]), np.float64)
    for b, r in enumerate(rows):
        out[r] += g[b]
    return out


def table_mean(table):
    return np.asarray(table, np.float64).mean(0, keepdims=True)


class RowCacheModel:
    """The write-back cache of d3ga_row_cache_select / _flush over any number of (table, stage) pairs (numpy arrays, changed
    in place)."""

    def __init__(self, pairs):
        self.pairs, self.prev, self.flag = pairs, -1, 0

    def _ok(self, i):
        return all(0 <= i < t.shape[0] for t, _ in self.pairs)

    def select(self, i):
        if not self._ok(i):
            self.flag = 1
            return
        if i == self.prev:
            return
        for t, s in self.pairs:
            if self.prev >= 0:
                t[self.prev] = s.reshape(t[self.prev].shape)
            s[...] = t[i].reshape(s.shape)
        self.prev = i

    def flush(self):
        if self.prev >= 0:
            for t, s in self.pairs:
                t[self.prev] = s.reshape(t[self.prev].shape)
