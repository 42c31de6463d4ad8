"""Float64 host replica of the device Philox draws (csrc/jets.h, walker_rev.h walker_draws,
quad_small.h, ecp.h k_ecp_rot / k_tmove).  numpy only, vectorised over stream ids.

A draw is a pure function of (seed, step, stream id, kind):
    counter = {sid, step lo, step hi, kind},  key = {seed lo, seed hi}
and Philox4x32-10 of it gives four 32-bit words.  The uniforms ((c >> 8) + 1) 2^-24 lie on the
24-bit grid in (0, 1] and are exact in float32 and float64 alike, so everything the device derives
from them without a transcendental (u, the rotation's sign, the T-move uniforms) is reproduced
bit for bit; the normals are Box-Muller in float64 here and in float with fast intrinsics on the
device, and agree to the device's rounding (tests/test_gpu_philox.py measures it).

Kinds: 0 gauss1, 1 gauss2, 2 u (one sweep of mc_step, sid = b N + e); 16, 17 the quaternion's
normals and 18 the sign of a walker's Haar rotation (sid = b); 19 the T-move selection uniform
(sid = b), 20 its acceptance uniforms (sid = b N + e).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57     # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85     # key schedule (Weyl) increments
MASK32 = 0xFFFFFFFF
GRID = 2.0 ** -24

KIND_GAUSS1, KIND_GAUSS2, KIND_U = 0, 1, 2
KIND_ROT_G, KIND_ROT_H, KIND_ROT_SIGN = 16, 17, 18
KIND_TM_SEL, KIND_TM_ACC = 19, 20


def philox4x32_10(counter, key):
    """Philox4x32-10: counter [4] and key [2] of 32-bit words (scalars or arrays that broadcast
    against each other) -> uint32 [4, ...]."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in counter]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(w, shape) for w in c]
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]     # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c).astype(np.uint32)


def words(seed, step, sid, kind):
    """The four output words [4, ...] of (seed, step, sid, kind); seed and step are 64-bit."""
    seed, step = int(seed), int(step)
    if not (0 <= seed < 2 ** 64 and 0 <= step < 2 ** 64):
        raise ValueError("seed and step are unsigned 64-bit")
    return philox4x32_10([sid, step & MASK32, step >> 32, kind], [seed & MASK32, seed >> 32])


def u4(seed, step, sid, kind):
    """Four uniforms [4, ...] on the 24-bit grid in (0, 1] (philox_u4), as float64."""
    return ((words(seed, step, sid, kind) >> np.uint32(8)).astype(np.float64) + 1.0) * GRID


def normal3(seed, step, sid, kind):
    """Three standard normals [3, ...]: Box-Muller on the four uniforms in float64, in the order
    of philox_normal3f (r0 cos, r0 sin, r1 cos)."""
    u = u4(seed, step, sid, kind)
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)])


def mc_draws(seed, offset, nsteps, B, N):
    """The draws of nsteps sweeps of mc_step: gauss1 [nsteps, B, 3N], gauss2 [nsteps, B, N, 3]
    (the electron-diagonal blocks) and u [nsteps, B, N] in [0, 1)."""
    sid = np.arange(B * N, dtype=np.uint64)
    g1 = np.empty((nsteps, B, 3 * N))
    g2 = np.empty((nsteps, B, N, 3))
    u = np.empty((nsteps, B, N))
    for st in range(nsteps):
        step = int(offset) + st
        g1[st] = normal3(seed, step, sid, KIND_GAUSS1).T.reshape(B, 3 * N)
        g2[st] = normal3(seed, step, sid, KIND_GAUSS2).T.reshape(B, N, 3)
        u[st] = (u4(seed, step, sid, KIND_U)[0] - GRID).reshape(B, N)
    return g1, g2, u


def haar_rotations(seed, step, B):
    """Haar O(3) matrices [B, 3, 3] as k_ecp_rot builds them: the unit quaternion (g0, g1, g2, h0)
    from the normals of kinds 16 and 17 gives SO(3), the sign -1 where kind 18's first uniform is
    below one half (compared as float32; the grid values are exact in it) makes it O(3)."""
    sid = np.arange(B, dtype=np.uint64)
    g = normal3(seed, step, sid, KIND_ROT_G)
    h = normal3(seed, step, sid, KIND_ROT_H)
    us = u4(seed, step, sid, KIND_ROT_SIGN)[0].astype(np.float32)
    w, x, y, z = g[0], g[1], g[2], h[0]
    n = 1.0 / np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w * n, x * n, y * n, z * n
    s = np.where(us < np.float32(0.5), -1.0, 1.0)
    m = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.ascontiguousarray(np.moveaxis(s * m, -1, 0))


def tmove_draws(seed, step, B, N):
    """The uniforms of k_tmove in [0, 1): u_sel [B] (selection) and u_acc [B, N] (acceptance)."""
    u_sel = u4(seed, step, np.arange(B, dtype=np.uint64), KIND_TM_SEL)[0] - GRID
    u_acc = (u4(seed, step, np.arange(B * N, dtype=np.uint64), KIND_TM_ACC)[0] - GRID).reshape(B, N)
    return u_sel, u_acc
