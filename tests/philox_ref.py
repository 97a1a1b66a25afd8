"""The restatement of tc_randn_clips (include/tooncrafter_hip.h) in numpy: Philox4x32-10 (Salmon et al., SC'11) in integers,
the uniforms u and v exactly, the normals in float64 -- and, for the error budget of the GPU test, the same formulas in
float32.  Pure numpy; what the CPU tests check the contract with and the GPU tests check the kernel against."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) c0..c3, key: two (k0, k1); returns the four output words as uint64 arrays
    holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in counter)
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2               # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words(seed, n, stream):
    """The n raw words of one clip: element 4q + m is word m of counter (q, 0, stream, 0) under key (lo32, hi32 of seed)."""
    seed, n, stream = int(seed), int(n), int(stream)
    assert 0 <= seed < 1 << 64 and 1 <= n <= 1 << 34 and 0 <= stream < 1 << 32
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(q)
    w = philox4x32_10((q, zero, zero + np.uint64(stream), zero), (seed & MASK32, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n].astype(np.uint32)


def uniforms(w):
    """(u of the even words, v of the odd words) of a word array of even length, exact in float64:
    u(w) = (2 (w >> 9) + 1) 2^-24 in [2^-24, 1 - 2^-24],  v(w) = (w >> 9) 2^-23 in [0, 1)."""
    w = np.asarray(w, dtype=np.uint64)
    u = (2.0 * (w[0::2] >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    v = (w[1::2] >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    return u, v


def _padded_words(seed, n, stream):
    return words(seed, ((n + 3) // 4) * 4, stream)


def normals(seed, n, stream):
    """float64 Box-Muller: z[2p] = r cos(2 pi v), z[2p + 1] = r sin(2 pi v), r = sqrt(-2 ln u), on word pairs (2p, 2p + 1)."""
    u, v = uniforms(_padded_words(seed, n, stream))
    r = np.sqrt(-2.0 * np.log(u))
    z = np.stack([r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)], axis=1).reshape(-1)
    return z[:n]


def normals_f32(seed, n, stream):
    """The same formulas with every operation in numpy float32 (u, v and 2 pi v's reduction aside: u and 2 v are exact in
    fp32, and cos / sin of pi * x are taken of the float32 product): the host's measure of what fp32 evaluation costs."""
    u, v = uniforms(_padded_words(seed, n, stream))
    u32, v2 = u.astype(np.float32), (2.0 * v).astype(np.float32)
    assert np.array_equal(u32.astype(np.float64), u) and np.array_equal(v2.astype(np.float64), 2.0 * v)
    r = np.sqrt(np.float32(-2.0) * np.log(u32))
    ang = np.float32(np.pi) * v2
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).reshape(-1)
    assert z.dtype == np.float32
    return z[:n]


def deviation(got, reference):
    """Largest |got - reference| relative to max(1, |reference|), in float64."""
    got, reference = np.asarray(got, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    return float((np.abs(got - reference) / np.maximum(1.0, np.abs(reference))).max())


def f32_deviation(seed, n, stream, reference=None):
    """What evaluating the formulas in float32 costs on this draw: `deviation` of normals_f32 from normals."""
    return deviation(normals_f32(seed, n, stream), normals(seed, n, stream) if reference is None else reference)


def rows(seeds, n, stream, fn=normals):
    return np.stack([fn(s, n, stream) for s in seeds])
