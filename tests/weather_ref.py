"""numpy restatements of the night, haze and rain ops of mx_weather_batch_u8, written from their
definitions in include/mx_det.h (a helper, not a test): Philox4x32-10, the three ops on uint8 [H, W, 3]
arrays, and the Box-Muller normal of the device generator. Every integer product is asserted to fit in
uint32, as the definitions promise; the two Random123 known answers of Philox are asserted on import."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
HAZE_TAG, RAIN_TAG, GAUSS_TAG = 0x48415A45, 0x5241494E, 0x5EED

KNOWN_ANSWERS = (  # (counter word, key word) -> output, Random123's kat_vectors for philox4x32 10
    ((0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
)


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) (arrays or ints, broadcast together) under the key
    (seed lo, seed hi): four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    for _ in range(10):
        p0 = c[0] * np.uint64(PHILOX_M0)
        p1 = c[2] * np.uint64(PHILOX_M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return [v.astype(np.uint32) for v in c]


def check_known_answers():
    for (cw, kw), want in KNOWN_ANSWERS:
        got = philox(cw, cw, cw, cw, kw | kw << 32)
        assert tuple(int(v) for v in got) == want, ([hex(int(v)) for v in got], [hex(v) for v in want])


check_known_answers()


def _u32(v):
    """v (uint64 array) after asserting that it fits in uint32."""
    assert int(np.max(v, initial=0)) <= M32
    return v


def gauss(seed, n):
    """The device generator's normals for the flat indices 0..n-1, in float64 from the same uniforms
    (the device evaluates log / cos / sqrt in f32: equal up to f32 rounding, not bit for bit)."""
    idx = np.arange(n, dtype=np.uint64)
    r = philox(idx & M32, idx >> np.uint64(32), GAUSS_TAG, 0, seed)
    u1 = ((r[0] >> 8).astype(np.float64) + 1.0) / 16777217.0
    u2 = (r[1] >> 8).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def night(img, gain, shot, read2, field):
    """op 1 with an explicit f32 field shaped like img: float32 throughout, one rounding per op."""
    f32 = np.float32
    v = img.astype(f32)
    d = v * f32(gain)
    s = np.sqrt(f32(shot) * d + f32(read2))
    assert d.dtype == f32 and s.dtype == f32
    o = d + s * np.asarray(field, dtype=f32)
    assert o.dtype == f32
    return np.clip(o, f32(0), f32(255)).astype(np.uint8)


def haze_alpha(H, W, lo, hi, seed):
    """The q16 alpha of every pixel of an H x W image: uint64 array [H, W]."""
    u = np.uint64
    y = np.arange(H, dtype=u)[:, None]
    x = np.arange(W, dtype=u)[None, :]
    S = np.zeros((H, W), dtype=u)
    for o in range(4):
        c, s = 256 >> o, 8 - o
        nj, ni = ((H - 1) >> s) + 2, ((W - 1) >> s) + 2
        L = (philox(np.arange(ni)[None, :], np.arange(nj)[:, None], HAZE_TAG, o, seed)[0] >> 16).astype(u)
        j, i = (y >> u(s)).astype(np.int64), (x >> u(s)).astype(np.int64)
        fy, fx = y & u(c - 1), x & u(c - 1)
        top = _u32(L[j, i] * (u(c) - fx) + L[j, i + 1] * fx)
        bot = _u32(L[j + 1, i] * (u(c) - fx) + L[j + 1, i + 1] * fx)
        S += u(8 >> o) * (_u32(top * (u(c) - fy) + bot * fy) >> u(2 * s))
    S16 = _u32(S * u(4369)) >> u(16)
    return u(lo) + (_u32(u(hi - lo) * S16) >> u(16))


def haze(img, lo, hi, air, seed):
    """op 2."""
    assert 0 <= lo <= hi <= 65535 and 0 <= air <= 255
    H, W, _ = img.shape
    alpha = haze_alpha(H, W, lo, hi, seed)[:, :, None]
    v = img.astype(np.uint64)
    out = _u32(v * (np.uint64(65536) - alpha) + np.uint64(air) * alpha + np.uint64(32768)) >> np.uint64(16)
    return out.astype(np.uint8)


def rain_heads(ys, xs, thr, seed):
    """The drop-head flags (0 / 1, int64) at rows ys x columns xs (int64 arrays; xs may be negative)."""
    X = xs.astype(np.int64)[None, :] + 4096
    assert X.min() >= 0
    w = philox(X >> 2, ys.astype(np.int64)[:, None], RAIN_TAG, 0, seed)
    lane = np.choose(X & 3, [v & 0xFFFF for v in w])
    return (lane < thr).astype(np.int64)


def rain_strength(H, W, thr, length, slant, fade, seed):
    """R of every pixel: int64 array [H, W] in 0..256."""
    assert 0 <= thr <= 65535 and 1 <= length <= 32 and -8 <= slant <= 8 and fade >= 0 and (length - 1) * fade < 256
    offs = [(k * slant) >> 3 for k in range(length)]  # Python's >> on ints is arithmetic
    xs = np.arange(min(offs), W + max(offs))
    heads = rain_heads(np.arange(H + length - 1), xs, thr, seed)
    R = np.zeros((H, W), dtype=np.int64)
    for k, off in enumerate(offs):
        c0 = off - min(offs)
        R = np.maximum(R, heads[k:k + H, c0:c0 + W] * (256 - k * fade))
    return R


def rain(img, thr, length, slant, fade, beta, seed):
    """op 3."""
    assert 0 <= beta <= 256
    H, W, _ = img.shape
    R = rain_strength(H, W, thr, length, slant, fade, seed)[:, :, None].astype(np.uint64)
    v = img.astype(np.uint64)
    return (v + (_u32((np.uint64(255) - v) * np.uint64(beta) * R) >> np.uint64(16))).astype(np.uint8)


def apply(img, spec, seed, field=None):
    """img under an ops.CorruptSpec-like (op code 5 night / 6 haze / 7 rain, parameters)."""
    op, p = int(spec[0]), spec[1]
    if op == 5:
        return night(img, p[0], p[1], p[2], field)
    if op == 6:
        return haze(img, p[0], p[1], p[2], seed)
    assert op == 7
    return rain(img, p[0], p[1], p[2], p[3], p[4], seed)
