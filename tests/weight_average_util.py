"""The numpy fp32 restatement of the weight-averaging update (pmgt_amd/ops/weight_average.hip: avg_apply) that the GPU tests compare with
bit for bit, and the inputs they share.  Every numpy operation below takes fp32 operands and rounds its result to fp32 once, which is
the kernel's contract: two products and one sum, three roundings, no fused multiply-add."""
import numpy as np

OP_SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4 * 256 * 3 + 1)      # tails, one block +- 1, four blocks + 1
CANARY = 64


def avg_apply_np(avg: np.ndarray, p: np.ndarray, w_old, w_new) -> np.ndarray:
    """avg * w_old + p * w_new in fp32, each operation rounded on its own."""
    avg, p = np.asarray(avg, dtype=np.float32), np.asarray(p, dtype=np.float32)
    a = avg * np.float32(w_old)
    b = p * np.float32(w_new)
    out = a + b
    assert a.dtype == b.dtype == out.dtype == np.float32
    return out


def swa_step_np(avg: np.ndarray, p: np.ndarray, models_num: int) -> np.ndarray:
    """swa_step for the model count AFTER its increment: beta = 1.0 / models_num in doubles, each weight rounded to fp32 once."""
    beta = 1.0 / int(models_num)
    return avg_apply_np(avg, p, np.float32(1.0 - beta), np.float32(beta))


def ema_replay_np(start: np.ndarray, snapshots, decay: float, warmup: bool, first_n: int = 0) -> np.ndarray:
    """The exponential average after one update per snapshot, from `start`, the decay series stated here independently of the package:
    d = decay, or min(decay, (1 + n) / (10 + n)) with warm-up, n counting from first_n."""
    avg = np.asarray(start, dtype=np.float32)
    for k, p in enumerate(snapshots):
        n = first_n + k
        d = min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)
        avg = avg_apply_np(avg, p, np.float32(d), np.float32(1.0 - d))
    return avg


def special_inputs(n: int, seed: int):
    """(avg, p): random normal values with +-0, 1e-30, 1e30 and equal-and-opposite pairs written over the first elements (as many as fit)."""
    rng = np.random.RandomState(seed)
    avg = rng.standard_normal(n).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    sa = np.array([0.0, -0.0, 1e-30, 1e30, 1.5, -2.25, 1e30, 0.0, -1e-30], dtype=np.float32)
    sp = np.array([-0.0, 0.0, 1e30, 1e-30, -1.5, 2.25, -1e30, 1e30, -1e30], dtype=np.float32)
    k = min(n, len(sa))
    # spread over the body and the tail: the last k elements, so that a short tail holds specials too
    if k:
        avg[n - k:] = sa[:k]
        p[n - k:] = sp[:k]
    return avg, p
