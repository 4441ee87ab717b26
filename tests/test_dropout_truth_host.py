"""The host restatement of csrc/dropout.hip (tests/dropout_truth.py) proved on the CPU: the Philox4x32-10 known-answer vectors,
the stream layout the GPU test relies on, the counter ranges BlockDrop.next_offset hands out, and the float32 helpers."""
from fractions import Fraction

import numpy as np

import dropout_truth as dt


def test_philox_known_answer_vectors():
    for ctr, key, want in dt.KAT:
        got = dt.philox4x32_10(*ctr, *key)
        assert tuple(int(g[0]) for g in got) == want, [hex(int(g[0])) for g in got]
    # vectorised evaluation = one evaluation per element
    c = np.array([k[0] for k in dt.KAT], dtype=np.uint64)
    same_key = dt.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], *dt.KAT[2][1])
    for i, row in enumerate(c):
        one = dt.philox4x32_10(*row, *dt.KAT[2][1])
        assert [int(w[i]) for w in same_key] == [int(w[0]) for w in one]


def test_counter_and_key_layout():
    """words() feeds Philox the counter (lo, hi, 0, 0) and the key (lo, hi); the counter carries into its second word and wraps."""
    seed = dt.BIG_SEED
    k = (seed & 0xFFFFFFFF, seed >> 32)
    assert k[1] != 0
    w = dt.words(seed, 2 ** 32 - 2, 4)
    for q, ctr in enumerate((2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)):
        one = dt.philox4x32_10(ctr & 0xFFFFFFFF, ctr >> 32, 0, 0, *k)
        assert [int(v) for v in w[q]] == [int(v[0]) for v in one]
    assert not np.array_equal(dt.words(seed, 0, 4), dt.words(seed & 0xFFFFFFFF, 0, 4)), "the high key word must matter"
    assert not np.array_equal(dt.words(seed, 2 ** 32, 1), dt.words(seed, 0, 1)), "the high counter word must matter"
    assert np.array_equal(dt.words(seed, 2 ** 64 - 1, 2)[1], dt.words(seed, 0, 1)[0])          # wraps mod 2^64
    assert np.array_equal(dt.words(seed, 5, 3, first=2), dt.words(seed, 7, 3))                 # stream property
    assert np.array_equal(dt.keep_mask(13, 0.5, seed, 3, first_elem=8), dt.keep_mask(21, 0.5, seed, 3)[8:])


def test_keep_rule():
    """The rule compares the word AFTER its rounding to float32 (24 bits): at p = 0.1 the threshold is T = float32(0.1) * 2^32, a
    multiple of the spacing 32 of float32 near it; T - 16 is a tie that goes to the even neighbour T - 32."""
    assert dt.keep_of_words(np.array([0, 1, 2 ** 32 - 1], dtype=np.uint64), 0.0).all()         # p = 0 keeps every word, 0 included
    T = int(Fraction(float(np.float32(0.1))) * 2 ** 32)
    assert T % 64 == 32
    w = np.array([T - 17, T - 16, T - 15, T, 0, 2 ** 32 - 1], dtype=np.uint64)
    assert list(dt.keep_of_words(w, 0.1)) == [0, 0, 1, 1, 0, 1]
    w = np.array([2 ** 31 - 129, 2 ** 31 - 128, 2 ** 31 - 1, 2 ** 31], dtype=np.uint64)      # spacing 128 below 2^31
    assert list(dt.keep_of_words(w, 0.5)) == [0, 0, 1, 1]


def test_inverse_keep_probability_is_unambiguous_at_the_tested_rates():
    """1 / (1 - p) in float32 arithmetic (the kernel) equals the float32 rounding of the float64 quotient at every rate used."""
    for p in (0.0, 0.1, 0.5, 0.3, 0.25):
        assert dt.inv_keep(p) == np.float32(1.0 / (1.0 - p)), p


def test_block_drop_offsets_are_disjoint():
    """Consecutive uses of one BlockDrop get consecutive, disjoint counter ranges of ceil(numel / 4) groups each."""
    from eventpretrain_amd import ops
    rd = ops.BlockDrop(drop=0.1, seed=3)
    numels = [5, 1, 8, 1023, 4, 3, 4096]
    seen = set()
    end = 0
    for n in numels:
        o = rd.next_offset(n)
        assert o == end                                      # no gap either: the stream is used densely
        groups = set(range(o, o + (n + 3) // 4))
        assert len(groups) * 4 >= n and not (groups & seen)
        seen |= groups
        end = o + (n + 3) // 4
    # the masks of two consecutive uses are two disjoint slices of ONE stream
    a, b = dt.keep_mask(5, 0.5, 3, 0), dt.keep_mask(8, 0.5, 3, 2)
    assert np.array_equal(np.concatenate([a, dt.keep_mask(3, 0.5, 3, 1)[:3], b])[[0, 1, 2, 3, 4, 8, 9]],
                          dt.keep_mask(16, 0.5, 3, 0)[[0, 1, 2, 3, 4, 8, 9]])


def test_boundary_draws():
    for kp in (0.7, 0.9, 0.5):
        d = dt.boundary_draws(kp)
        t = np.float32(1) - np.float32(kp)
        assert np.nextafter(d["neighbours"][0], np.float32(1)) == t == np.nextafter(d["neighbours"][1], np.float32(0))
        assert np.nextafter(d["straddle"][0], np.float32(1)) == d["straddle"][1]
        s = dt.rows_factor(d["straddle"], kp, 2)
        assert s[0] == 0 and s[1] == np.float32(1) / np.float32(kp)          # one sample dropped, the next kept
        # the sum kp + u rounds at the spacing of 1.0, which is where the float32 boundary can sit away from 1 - kp
        assert abs(float(d["straddle"][1]) - float(t)) <= float(np.spacing(np.float32(1)))
    assert (dt.rows_factor(None, 0.7, 3) == 1).all() and (dt.rows_factor(np.zeros(3, np.float32), 1.0, 3) == 1).all()


def test_single_rounding_fma_against_exact_rationals():
    rng = np.random.default_rng(5)
    n = 600
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * rng.choice([1e-6, 1.0, 1e4], n)).astype(np.float32)
    # planted double-rounding traps: a * b = 1 + 2^-11 + 2^-24 sits half-way between two float32 values (nearest-even goes down),
    # c is far below float64's reach and decides the side
    a[:2], b[:2], c[:2] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), [2.0 ** -80, -2.0 ** -80]
    got = dt.fma_f32(a, b, c)
    for i in range(n):
        ex = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(ex))
        cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
        dist = [abs(Fraction(float(z)) - ex) for z in cands]
        assert got[i] == cands[dist.index(min(dist))], i
    assert got[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and got[1] == np.float32(1 + 2.0 ** -11)
