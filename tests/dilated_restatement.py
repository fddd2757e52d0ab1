"""The random dilation of a kNN graph (crfconv_graph_table_dilated) restated in numpy from its specification, not from the kernel:
uint64 arithmetic with wrap-around, one row at a time where it matters, vectorised over the picks.

Per row i of nbr [n, K]: valid = the entries inside [0, n_src) in column order, have = |valid|, n_pick = min(k_pick, have); pick t is
valid[((h(i, t) >> 32) * have) >> 32]; modes 1 and 2 then drop the picks equal to i; mode 2 appends the arange loops."""
import numpy as np

MASK = (1 << 64) - 1
DIL_DOMAIN = 0xA0761D6478BD642F
U = np.uint64


def key_of(seed, counter, salt):
    """The part of the hash input that a launch shares (Python integers, mod 2^64)."""
    return ((int(seed) & MASK) ^ DIL_DOMAIN) + 0x9E3779B97F4A7C15 * (int(counter) + 1) + int(salt) * 0xC2B2AE3D27D4EB4F & MASK


def hashes(key, slots):
    """h for an array of slot numbers 64 i + t (uint64), splitmix64's finisher."""
    with np.errstate(over='ignore'):
        z = U(key) + slots.astype(U) * U(0xD1B54A32D192ED03)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def slots_of(key, rows, n_pick, have):
    """slot_t for t < n_pick of every row in `rows` with `have` valid entries each: int64 [len(rows), n_pick].  The product of a 32-bit
    and an at most 7-bit number stays far below 2^64."""
    t = np.arange(n_pick, dtype=U)[None, :]
    h = hashes(key, np.asarray(rows, dtype=U)[:, None] * U(64) + t)
    return (((h >> U(32)) * U(have)) >> U(32)).astype(np.int64)


def picks_of(nbr, n_src, k_pick, seed, counter, salt):
    """Per row the int64 array of its n_pick picks, before any self filter."""
    nbr = np.asarray(nbr)
    key = key_of(seed, counter, salt)
    picks = []
    for i in range(nbr.shape[0]):
        entries = nbr[i]
        valid = entries[(entries >= 0) & (entries < n_src)].astype(np.int64)
        n_pick = min(k_pick, valid.size)
        picks.append(valid[slots_of(key, [i], n_pick, valid.size)[0]] if n_pick else np.zeros(0, dtype=np.int64))
    return picks


def edges_of(picks, self_mode):
    """(row, col) int64: the picks in row-major pick order, those equal to their row dropped under modes 1 and 2, the arange loops
    appended under mode 2."""
    n = len(picks)
    kept = [p[p != i] if self_mode else p for i, p in enumerate(picks)]
    row = np.concatenate([np.full(p.size, i, dtype=np.int64) for i, p in enumerate(kept)] + [np.zeros(0, dtype=np.int64)])
    col = np.concatenate(kept + [np.zeros(0, dtype=np.int64)])
    if self_mode == 2:
        loops = np.arange(n, dtype=np.int64)
        row, col = np.concatenate([row, loops]), np.concatenate([col, loops])
    return row, col


def dilate(nbr, n_src, k_pick, seed, counter, salt, self_mode):
    """-> (picks, row, col): picks_of and the edge list edges_of makes of them."""
    picks = picks_of(nbr, n_src, k_pick, seed, counter, salt)
    return (picks,) + edges_of(picks, self_mode)
