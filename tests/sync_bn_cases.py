"""Shared by the synchronised-BatchNorm tests: the case table of the kernel-level test and a NumPy fp64 restatement of what the
ranks exchange -- per-shard moments ``[C means | C M2 | count]`` and their merge by Chan's pairwise update in rank order
(include/zsv_hip.h, zsv_bn_sync_finalize).  tests/test_sync_bn_host.py pins the restatement against ``np.var`` of the
concatenation, so the expectations of the GPU tests are themselves pinned.  Plain module: no fixtures, no device."""
import numpy as np

# (N, C, spatial), shard splits along N
CASES = [
    ((5, 5, (3, 4, 4)), ([1, 4], [2, 2, 1])),        # float4 route, odd C, three ranks
    ((4, 45, (2, 7, 7)), ([1, 3],)),                 # S % 4 != 0
    ((3, 130, (2, 7, 7)), ([1, 1, 1],)),             # C above 128
    ((4, 7, (1, 1, 1)), ([1, 3], [2, 2])),           # a shard with one value per channel: local M2 = 0
    ((6, 64, (4, 8, 8)), ([2, 4], [6])),             # world 1
]


def shard_moments(x):
    """One rank's row for an (N, C, ...) array: C means, C sums of squared deviations from them, the count N*S (fp64)."""
    x = np.asarray(x, dtype=np.float64)
    c = x.shape[1]
    flat = np.moveaxis(x, 1, 0).reshape(c, -1)
    n = flat.shape[1]
    if n == 0:
        return np.zeros(2 * c + 1)
    mean = flat.mean(axis=1)
    m2 = ((flat - mean[:, None]) ** 2).sum(axis=1)
    return np.concatenate([mean, m2, [float(n)]])


def merge_moments(rows):
    """``rows``: (world, 2C+1) in rank order -> (mean (C,), M2 (C,), count): n = n_a + n_b, delta = mean_b - mean_a,
    mean += delta * n_b / n, M2 += M2_b + delta^2 * n_a * n_b / n; a rank whose count is 0 contributes nothing."""
    rows = np.asarray(rows, dtype=np.float64)
    c = (rows.shape[1] - 1) // 2
    n, mean, m2 = 0.0, np.zeros(c), np.zeros(c)
    for row in rows:
        nb = row[2 * c]
        if nb <= 0:
            continue
        if n == 0:
            n, mean, m2 = nb, row[:c].copy(), row[c:2 * c].copy()
            continue
        tot = n + nb
        delta = row[:c] - mean
        mean = mean + delta * nb / tot
        m2 = m2 + row[c:2 * c] + delta * delta * n * nb / tot
        n = tot
    return mean, m2, n


def split(t, sizes):
    """Consecutive parts of ``t`` along axis 0 with the given sizes."""
    out, at = [], 0
    for k in sizes:
        out.append(t[at:at + k])
        at += k
    assert at == len(t)
    return out
