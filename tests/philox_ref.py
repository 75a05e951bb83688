"""A reference for the library's noise stream that shares no code with it: Philox4x32-10 in numpy uint64 arithmetic (Salmon et
al. 2011; pinned to the Random123 known answers by tests/test_philox_ref.py), the documented keying (noise section),
Box-Muller in float64, the element -> (group, lane) maps of the three tensors, and the masks from the oracle's mask helpers.

    counter = (group, low32(b), draw, high32(b)),  b = sample_offset + batch index (mod 2^64)
    key     = (low32(seed), high32(seed))
    draw    = base + {x: 0, adj: 1, rank2: 2};  base = 0 for the prior, 3 + 3 (step * per_step + phase) for a half-step,
              per_step = n_steps + 1 (3 for S4)
"""
import numpy as np
import torch

from oracle import ccsd_oracle as O

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TARGETS = {"x": 0, "adj": 1, "rank2": 2}


def philox4x32_10(counter, key):
    """counter: (..., 4), key: (..., 2) arrays of 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    c = np.asarray(counter).astype(np.uint64) & LO
    k = np.asarray(key).astype(np.uint64) & LO
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bit products: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def draw_base(step, phase, per_step):
    """Draw id of target x of half-step (step, phase); None = the prior."""
    return 0 if step is None else 3 + 3 * (step * per_step + phase)


def per_step(predictor, n_steps):
    return 3 if predictor == "S4" else n_steps + 1


def normals(group, b, draw, seed):
    """The four float64 standard normals of Philox group `group` (array) of global sample index b, draw id `draw`: (..., 4)."""
    g = np.asarray(group, dtype=np.uint64)
    b = int(b) % (1 << 64)
    seed = int(seed) % (1 << 64)
    ctr = np.stack([g, np.full_like(g, b & 0xFFFFFFFF), np.full_like(g, int(draw)), np.full_like(g, b >> 32)], -1)
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    out = np.empty(r.shape, np.float64)
    for h in (0, 1):
        u1 = ((r[..., 2 * h] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24      # (0, 1]
        u2 = (r[..., 2 * h + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                   # [0, 1)
        rad = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * h] = rad * np.cos(2.0 * np.pi * u2)
        out[..., 2 * h + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out


def _flat(n, b, draw, seed):
    """Raw draws of flat element indices 0 .. n - 1: group idx >> 2, lane idx & 3 (each group generated once)."""
    return normals(np.arange((n + 3) >> 2), b, draw, seed).reshape(-1)[:n]


def raw_x(N, F, b, draw, seed):
    return _flat(N * F, b, draw, seed).reshape(N, F)


def raw_adj(N, b, draw, seed):
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    z = _flat(N * N, b, draw, seed)[np.minimum(i, j) * N + np.maximum(i, j)]
    z[i == j] = 0.0
    return z


def raw_rank2(E, K, b, draw, seed, flat):
    if flat:                                           # four consecutive elements of the flattened block
        return _flat(E * K, b, draw, seed).reshape(E, K)
    EG = (E + 3) >> 2                                  # group (e >> 2) K + k, lane e & 3: four consecutive edge rows of one column
    n = normals(np.arange(EG * K), b, draw, seed).reshape(EG, K, 4)
    return np.ascontiguousarray(n.transpose(0, 2, 1)).reshape(4 * EG, K)[:E]


_masks = {}


def masks(flags, N, F, is_cc, d_min, d_max):
    """[x, adj, rank2 or None] 0 / 1 float64 arrays: the oracle's masks of a batch; adj also 0 on the diagonal (symmetric noise has none)."""
    flags = torch.as_tensor(flags, dtype=torch.float32)
    key = (N, F, is_cc, d_min, d_max, flags.numpy().tobytes())
    if key not in _masks:
        _masks.clear()                                  # (one batch at a time: a rank2 mask can take hundreds of megabytes)
        _masks[key] = _build_masks(flags, N, F, is_cc, d_min, d_max)
    return _masks[key]


def _build_masks(flags, N, F, is_cc, d_min, d_max):
    B = flags.shape[0]
    one = lambda shape: torch.ones(shape, dtype=torch.float32)
    mx = O.mask_x(one((B, N, F)), flags).numpy().astype(np.float64)
    ma = O.mask_adjs(one((B, N, N)), flags).numpy().astype(np.float64) * (1.0 - np.eye(N))
    mr = None
    if is_cc:
        fl, fr = O.rank2_flags(flags, N, d_min, d_max)
        mr = (fl[:, :, None] * fr[:, None, :]).numpy().astype(np.float64)
    return [mx, ma, mr]


def masked_draws(flags, N, F, is_cc, d_min, d_max, base, seed, sample_offset, flat):
    """([x, adj, rank2 or None] float64 arrays, their masks): what ccsd_init_state (base 0) / ccsd_noise_draws must write for a
    batch.  (The draws of a sample whose mask is 0 everywhere are not generated: 0 times anything finite.)"""
    m = masks(flags, N, F, is_cc, d_min, d_max)
    B = m[0].shape[0]
    E, K = O.get_rank2_dim(N, d_min, d_max) if is_cc else (0, 0)
    raw = [lambda b: raw_x(N, F, b, base + 0, seed), lambda b: raw_adj(N, b, base + 1, seed),
           lambda b: raw_rank2(E, K, b, base + 2, seed, flat)]
    out = []
    for mt, fn in zip(m, raw):
        if mt is None:
            out.append(None)
            continue
        v = np.zeros_like(mt)
        for b in range(B):
            if mt[b].any():
                v[b] = fn(sample_offset + b) * mt[b]
        out.append(v)
    return out, m
