"""How the training pieces' references (train_block_ref.py, train_attn_ref.py, train_stem_ref.py, train_heads_ref.py) measure a
deviation and what they allow: one definition for the four."""
import numpy as np

FLOOR, FACTOR = 1e-6, 4.0


def dev(got, ref):
    """Largest absolute difference over the reference's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())


def deviations(got, ref, quantities):
    return {q: dev(got[q], ref[q]) for q in quantities}


def bound(own):
    """What a kernel may deviate from float64, given what float32 torch deviates on the same inputs."""
    return max(FACTOR * own, FLOOR)
