"""The stochastic regularisers of csrc/dropout.hip restated on the host, bit for bit: the Philox4x32-10 stream of evp_dropout_fwd,
its keep rule and output arithmetic, evp_dropout_apply, and the per-sample factor of evp_rows_scale_f32. Everything here is
integer or float32 arithmetic in numpy, so the GPU tests compare with `==` and carry no tolerance.

The stream (who draws which word) is this build's own definition, pinned here; it is not timm's / torch's:
  group q of a launch takes the counter ctr = offset + q (mod 2^64) as (ctr & 0xffffffff, ctr >> 32, 0, 0),
  the key is (seed & 0xffffffff, seed >> 32), seed = host seed + device scalar (mod 2^64),
  element 4q + i takes output word i and is kept when float32(word) * 2^-32 >= float32(p)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)        # Philox4x32 multipliers (Salmon et al. 2011)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)        # Weyl key increments
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
BIG_SEED = 0x0123456789ABCDEF                                # both key words non-zero
GRID_GROUPS = 16384 * 256                                    # one pass of the largest grid (grid_for: 16,384 blocks x 256 threads)

# Philox4x32-10 known-answer vectors (Random123 kat_vectors): counter words, key words, output words
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays (or scalars) that hold 32-bit words -> the four output words, uint64 arrays < 2^32."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                            # 32 x 32 -> 64 bits: no overflow in uint64
        n0, n2 = (p1 >> S32) ^ c1 ^ k0, (p0 >> S32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & LO, p0 & LO, n0, n2
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return c0, c1, c2, c3


def words(seed, offset, n_groups, first=0):
    """[n_groups, 4] uint64: the words of groups first .. first + n_groups - 1 of a launch with (seed, offset)."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    q = np.arange(first, first + n_groups, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset) + q                          # wraps mod 2^64 like the kernel's uint64_t
    z = np.zeros_like(ctr)
    return np.stack(philox4x32_10(ctr & LO, ctr >> S32, z, z, seed & 0xFFFFFFFF, seed >> 32), axis=1)


def keep_of_words(w, p):
    """keep rule on words of any shape -> uint8 0/1."""
    u = w.astype(np.float32) * np.float32(2.0 ** -32)        # uint -> float32 rounds to nearest even, like the device conversion
    return (u >= np.float32(p)).astype(np.uint8)


def keep_mask(n, p, seed, offset, first_elem=0):
    """uint8 [n]: the mask of elements first_elem .. first_elem + n - 1 of a launch (first_elem % 4 == 0)."""
    assert first_elem % 4 == 0
    g = (n + 3) // 4
    return keep_of_words(words(seed, offset, g, first_elem // 4), p).reshape(-1)[:n]


def inv_keep(p):
    """float32 1 / (1 - p), in the kernel's float32 arithmetic."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_out(x32, mask, scale):
    """float32 x * scale where mask, +0 elsewhere (x32: float32 array holding the kernel's input values)."""
    return np.where(mask != 0, x32.astype(np.float32) * np.float32(scale), np.float32(0.0)).astype(np.float32)


# ---- evp_rows_scale_f32 ----------------------------------------------------------------------------------------------------------
def rows_factor(u, kp, n_samples):
    """float32 [n_samples]: s_b = floor(float32(kp) + u_b) / kp in float32; 1 when u is None or kp >= 1."""
    kp = np.float32(kp)
    if u is None or kp >= np.float32(1.0):
        return np.ones(n_samples, dtype=np.float32)
    return (np.floor(kp + u.astype(np.float32)) / kp).astype(np.float32)


def boundary_draws(kp):
    """{name: float32 [2]} pairs of ADJACENT float32 draws around the drop / keep boundary 1 - kp.
    "neighbours": the two float32 neighbours of float32(1) - float32(kp). In float32, kp + u rounds, so both of them may land on
    the same side; "straddle" is therefore the adjacent pair (largest dropped draw, smallest kept draw) found by walking."""
    kp = np.float32(kp)
    t = np.float32(1.0) - kp
    one, zero = np.float32(1.0), np.float32(0.0)
    u = np.nextafter(t, zero)
    for _ in range(8):                                       # step down until dropped ...
        if np.floor(kp + u) == 0:
            break
        u = np.nextafter(u, zero)
    while np.floor(kp + np.nextafter(u, one)) == 0:          # ... then up to the last dropped draw
        u = np.nextafter(u, one)
    return {"neighbours": np.array([np.nextafter(t, zero), np.nextafter(t, one)], dtype=np.float32),
            "straddle": np.array([u, np.nextafter(u, one)], dtype=np.float32)}


def fma_f32(a, b, c):
    """RN_float32(a * b + c) with ONE rounding, for float32 arrays. a * b is exact in float64 (24 + 24 bits); the float64 sum t can
    round. Rounding to float64 is monotone and every float32 mid-point is a float64, so t and the exact sum round to the same
    float32 unless t IS a mid-point while the part it lost (recovered by TwoSum) is non-zero: that part then decides the side."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)                          # p + c == t + err exactly
    f = t.astype(np.float32)
    f64 = f.astype(np.float64)
    lo = np.where(f64 <= t, f, np.nextafter(f, np.float32(-np.inf)))
    hi = np.where(f64 >= t, f, np.nextafter(f, np.float32(np.inf)))
    mid = (f64 != t) & ((t - lo.astype(np.float64)) == (hi.astype(np.float64) - t))
    return np.where(mid & (err > 0), hi, np.where(mid & (err < 0), lo, f)).astype(np.float32)


def rows_scale_truth(x, u, kp, rps, res):
    """-> (prod, fused, unfused): prod = float32(s_b * x) is `out` without res and what lp rounds; with res, `out`
    must equal one of fused = RN(x * s + res) and unfused = RN(RN(x * s) + res)."""
    M = x.shape[0]
    s = np.repeat(rows_factor(u, kp, (M + rps - 1) // rps), rps)[:M, None].astype(np.float32)
    prod = (x.astype(np.float32) * s).astype(np.float32)
    if res is None:
        return prod, None, None
    fused = fma_f32(x, np.broadcast_to(s, x.shape), res)
    unfused = (prod + res.astype(np.float32)).astype(np.float32)
    return prod, fused, unfused
