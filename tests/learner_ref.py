"""The native learner's dropout contract (include/az_train.h, "DROPOUT") restated in numpy uint64: the device generator's
mixing function and streams (csrc/dev_rng.h), the threshold, the factor and which draw decides which element.  Written
from the header's statement, not from the kernel."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
LEARN_STREAM = 0x4C52
KEEP_ATTN, KEEP_POLICY, KEEP_POOL = 8, 9, 10        # tensor ids; block k is k
CH, HEADS, TOKENS, COLS = 64, 4, 42, 7


def mix64(x):
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def stream_state(seed, call, a, b):
    """DevRng(seed, call, a, b).s for an array of group indices a."""
    a = np.asarray(a, np.uint64)
    with np.errstate(over="ignore"):
        inner = mix64(np.uint64(call) + GOLDEN * (a + np.uint64(1)))
        return mix64(np.uint64(seed) ^ inner ^ np.uint64(int(b) << 32))


def draws(seed, call, groups, tensor, count):
    """uint32 [len(groups), count]: draw j of the stream (seed, call, group, LEARN_STREAM + tensor)."""
    s0 = stream_state(seed, call, groups, LEARN_STREAM + tensor)
    with np.errstate(over="ignore"):
        steps = (np.arange(count, dtype=np.uint64) + np.uint64(1)) * GOLDEN
        return (mix64(s0[:, None] + steps[None, :]) >> np.uint64(32)).astype(np.uint32)


def thr(p):
    """(uint32) floor(p * 2^32 + 0.5) in double; 2^32 counts as 2^32 - 1."""
    return min(int(np.floor(float(p) * 4294967296.0 + 0.5)), 0xFFFFFFFF)


def factor(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_factors(seed, call, n_groups, tensor, p, first=0):
    """float32 [n_groups, 64]: 0 or factor(p) per element, group a = first .. first + n_groups - 1."""
    d = draws(seed, call, np.arange(first, first + n_groups), tensor, CH)
    return np.where(d >= np.uint32(thr(p)), factor(p), np.float32(0.0)).astype(np.float32)


def keep_bits(seed, call, n, p):
    """uint64 [n, 4, 42]: bit j of word (n, h, i) from draw j of group (4 n + h) * 42 + i; bits 42 .. 63 zero."""
    d = draws(seed, call, np.arange(n * HEADS * TOKENS), KEEP_ATTN, TOKENS)
    kept = (d >= np.uint32(thr(p))).astype(np.uint64)
    words = (kept << np.arange(TOKENS, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)
    return words.reshape(n, HEADS, TOKENS)


def keeps(seed, call, n, n_blocks, rates):
    """What k_learn_keep writes for a batch of n rows at rates (block, attention, policy, pool); None where the rate is 0."""
    p_block, p_attn, p_policy, p_pool = rates
    return dict(blocks=[keep_factors(seed, call, n, k, p_block) for k in range(n_blocks)] if p_block > 0 else None,
                attn=keep_bits(seed, call, n, p_attn) if p_attn > 0 else None,
                policy=keep_factors(seed, call, n * COLS, KEEP_POLICY, p_policy).reshape(n, COLS, CH) if p_policy > 0 else None,
                pool=keep_factors(seed, call, n, KEEP_POOL, p_pool) if p_pool > 0 else None)
