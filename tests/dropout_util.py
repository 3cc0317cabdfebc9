"""Numpy restatement of the counter-based dropout RNG of the HIP kernels (pmgt_amd/csrc/common.h: fmix32, make_drop_key, drop_keep4,
site_id) and of the two draws of nfr_generate_kernel (pmgt_amd/csrc/loss.hip), bit for bit in uint32 arithmetic, so that a CPU reference
can apply exactly the masks a kernel draws.  test_dropout_entries_gpu.py compares it with the device (pmgt_op_dropout_keep,
pmgt_op_nfr_generate); everything else that runs with dropout on builds its reference masks from `keep`.

The keep decision: one hash pair (x, y) per (row, column group of 4); element c of a row uses the 16-bit lane c & 3 of group c >> 2 and is
kept when lane >= thr >> 16, thr = (uint32)(double(float32 p) * 2^32) saturated.  The effective drop probability is therefore
(thr >> 16) / 65536 (p = 0.1 -> 6553 / 65536 = 0.09999), while the survivors are scaled by 1 / (1 - float32 p)."""
import numpy as np

M32 = 0xFFFFFFFF
SITE_EMB, SITE_A1, SITE_A2, SITE_AO, SITE_FO, SITE_NFR1, SITE_NFR2 = range(7)


def site_id(layer, kind):
    """layer -1 = the embedding / the NFR draws, 0 .. L-1 = encoder layers."""
    return ((layer + 1) * 8 + kind) & M32


def fmix32(h):
    """murmur3 finaliser on a Python int or a uint32 array."""
    if isinstance(h, np.ndarray):
        h = h.astype(np.uint32, copy=True)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
        return h
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def drop_threshold(p):
    t = float(np.float32(p)) * 4294967296.0
    return M32 if t >= 4294967295.0 else int(t)


def drop_scale(p):
    """What a kept element is multiplied by: fp32 1 / (1 - p)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def make_drop_key(seed, step, site, p):
    """(k0, k1, thr) of make_drop_key; seed / step as the int64 values of the engine's rng_state (negative = top bit set)."""
    seed, step, site = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(site) & M32
    k0 = fmix32((seed & M32) ^ ((site * 0x9E3779B1) & M32))
    k1 = fmix32(((seed >> 32) + (step & M32) * 0x7FEB352D + (step >> 32) + site) & M32)
    return k0, k1, drop_threshold(p)


def keep(seed, step, site, rows, cols, p):
    """bool [rows, cols]: True where the kernels keep element (row, col) of dropout site `site`.  `rows`: a count (rows 0 .. rows-1) or
    an array of row indices."""
    r = np.arange(rows, dtype=np.uint32) if np.isscalar(rows) else (np.asarray(rows).astype(np.int64) & M32).astype(np.uint32)
    if not float(np.float32(p)) > 0.0:
        return np.ones((r.size, cols), dtype=bool)
    k0, k1, thr = make_drop_key(seed, step, site, p)
    ncg = (cols + 3) // 4
    cg = np.arange(ncg, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = r[:, None] * np.uint32(0x9E3779B1) + cg[None, :] * np.uint32(0x85EBCA77) + np.uint32(k0)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x2C1B3C6D)
        x ^= x >> np.uint32(12)
        y = x * np.uint32(0x297A2D39) + np.uint32(k1)
        y ^= y >> np.uint32(15)
    t = np.uint32(thr >> 16)
    out = np.empty((r.size, ncg, 4), dtype=bool)
    out[:, :, 0] = (x & np.uint32(0xFFFF)) >= t
    out[:, :, 1] = (x >> np.uint32(16)) >= t
    out[:, :, 2] = (y & np.uint32(0xFFFF)) >= t
    out[:, :, 3] = (y >> np.uint32(16)) >= t
    return out.reshape(r.size, ncg * 4)[:, :cols]


def _nfr_u32(k0, k1, i):
    """The `u32` lambda of nfr_generate_kernel; i: uint64 array."""
    with np.errstate(over="ignore"):
        lo = (i & np.uint64(M32)).astype(np.uint32)
        hi = (i >> np.uint64(32)).astype(np.uint32)
        x = fmix32((lo ^ np.uint32(k0)) * np.uint32(0x9E3779B1) + hi)
        return fmix32(x + np.uint32(k1))


def nfr_device_masks(ids, n_nodes, seed, step, random_ratio, mask_ratio):
    """ids [B, S] int64 -> (masked_ids, tgt_full) as nfr_generate_kernel writes them: position 0 and padding (id 0) untouched; with
    probability random_ratio the id is replaced by a uniform node in [2, n_nodes + 2); then with probability mask_ratio the (possibly
    replaced) id becomes the target and the position is set to 1 (<mask>); tgt_full is -1 where nothing is to be reconstructed."""
    ids = np.asarray(ids, dtype=np.int64)
    B, S = ids.shape
    idx = np.arange(B * S, dtype=np.uint64).reshape(B, S)
    a0, a1, _ = make_drop_key(seed, step, SITE_NFR1, 0.5)
    b0, b1, _ = make_drop_key(seed, step, SITE_NFR2, 0.5)
    inv24 = np.float32(1.0 / 16777216.0)
    r1 = (_nfr_u32(a0, a1, np.uint64(2) * idx) >> np.uint32(8)).astype(np.float32) * inv24
    repl = np.int64(2) + (_nfr_u32(a0, a1, np.uint64(2) * idx + np.uint64(1)) % np.uint32(n_nodes)).astype(np.int64)
    r2 = (_nfr_u32(b0, b1, idx) >> np.uint32(8)).astype(np.float32) * inv24
    live = (ids != 0) & (np.arange(S)[None, :] > 0)
    masked = np.where(live & (r1 < np.float32(random_ratio)), repl, ids)
    hit = live & (r2 < np.float32(mask_ratio))
    tgt = np.where(hit, masked, np.int64(-1))
    masked = np.where(hit, np.int64(1), masked)
    return masked.astype(np.int64), tgt.astype(np.int64)


def need_rows(B, P, S, nfr_rows):
    """The compact row list of the last layer of the shortcut path (build_need_rows): CLS rows of the B targets, of the P pairs, then the
    masked rows in their given order."""
    return np.concatenate([np.arange(B + P, dtype=np.int64) * S, np.asarray(nfr_rows, dtype=np.int64)])
