"""Cloud::subsample's seeded draw stream (gpd_amd/csrc/sample_model.h), restated in pure Python for the tests:
xorshift64 from 0x9E3779B97F4A7C15 ^ seed with the steps << 13, >> 7, << 17."""
import numpy as np

MASK = (1 << 64) - 1


def stream(seed):
    s = 0x9E3779B97F4A7C15 ^ (seed & 0xFFFFFFFF)
    while True:
        s ^= (s << 13) & MASK
        s ^= s >> 7
        s ^= (s << 17) & MASK
        yield s


def with_repetition(n, num_draws, seed):
    """Positions into a list of n sample indices: num_draws >= n keeps the list in order, else num_draws draws next() % n."""
    if num_draws <= 0:
        return np.zeros(0, np.int32)
    if num_draws >= n:
        return np.arange(n, dtype=np.int32)
    g = stream(seed)
    return np.array([next(g) % n for _ in range(num_draws)], np.int32)


def dense_fisher_yates(n, num_draws, seed):
    """The mirror's subsampleUniformly as it was before the stream had a header of its own: an n-sized array,
    min(num_draws, n) swaps, the first that many entries."""
    if num_draws <= 0:
        return np.zeros(0, np.int32)
    idx = list(range(n))
    m = min(num_draws, n)
    g = stream(seed)
    for i in range(m):
        j = i + next(g) % (n - i)
        idx[i], idx[j] = idx[j], idx[i]
    return np.array(idx[:m], np.int32)
