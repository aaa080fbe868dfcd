"""fp64 / numpy restatement of what makani_amd/csrc/noise.hip computes: the generator (Philox4x32-10, the uniform mapping,
Box-Muller, the group / offset layout of the counter) and the three update rules (white, autoregressive, replace).  Written
from the published algorithm (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the formulas of
makani/models/noise.py; shares no code with the kernel."""
import json
import os

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two ints -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def uniforms(xa, xb):
    """u1 in (0, 1], u2 in [0, 1): 24-bit, exactly representable in fp32"""
    u1 = ((xa >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (xb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def box_muller(xa, xb):
    u1, u2 = uniforms(xa, xb)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def normals(seed, offset, n, first_group=0):
    """the n standard normals (fp64) of ONE time level: element e belongs to group e // 4, lane e % 4"""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    groups = (n + 3) // 4
    g = np.arange(first_group, first_group + groups, dtype=np.uint64)
    x = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32), offset & MASK32, offset >> 32), (seed & MASK32, seed >> 32))
    z0, z1 = box_muller(x[0], x[1])
    z2, z3 = box_muller(x[2], x[3])
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[:n]


def draw(seed, offset, levels, B, inner):
    """innovations (B, levels, *inner) fp64: level t is drawn at offset + t over the flattened (B, *inner)"""
    n = B * int(np.prod(inner))
    return np.stack([normals(seed, offset + t, n).reshape(B, *inner) for t in range(levels)], axis=1)


def update(state, xi, mode, sigma=None, phi=None, reflect=False):
    """state (B, T, C, L, M, 2), xi (B, T or 1, C, L, M, 2), sigma (C, L), phi (C), all fp64 -> the new state"""
    s = -1.0 if reflect else 1.0
    if mode == "white":
        return s * xi
    sg = sigma[None, None, :, :, None, None]
    ph = phi[None, None, :, None, None, None]
    eta = s * sg * xi
    if mode == "ar":
        return np.concatenate([state[:, 1:], ph * state[:, -1:] + eta], axis=1)
    assert mode == "replace"
    new = np.empty_like(eta)
    new[:, 0] = eta[:, 0] / np.sqrt(1.0 - ph[:, 0] ** 2)
    for t in range(1, eta.shape[1]):
        new[:, t] = ph[:, 0] * new[:, t - 1] + eta[:, t]
    return new


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


# ---- the fixtures recorded from the reference's own classes (tools/make_noise_golden.py) -------------------------------
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise.npz")
GOLDEN = np.load(GOLDEN_PATH, allow_pickle=False) if os.path.exists(GOLDEN_PATH) else None        # (None: not recorded yet)
CASES = sorted({k.split("/")[0] for k in GOLDEN.files}) if GOLDEN is not None else []


def build_case(case):
    """the package's module (on the CPU) for a recorded case, and the case's settings"""
    import makani_amd as ma
    meta = json.loads(str(GOLDEN[f"{case}/meta"]))
    return getattr(ma, meta["cls"])(batch_size=meta["batch_size"], **meta["kwargs"]), meta
