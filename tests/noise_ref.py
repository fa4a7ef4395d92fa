"""The seeded standard-normal draws of include/epiekf.h, restated twice: in NumPy here (whole arrays at a
time, every written operation one rounding: NumPy never contracts) and in C (tests/noise_ref.c, one draw at a time), which
NoiseRef builds and loads.  Neither shares code with csrc/noise.hpp."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "noise_ref.c")
M32 = np.uint64(0xFFFFFFFF)

A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
     1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
     5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
CC = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
     6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
     2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
     1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counter words (uint64 arrays holding 32-bit values) -> the four output words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def uniform(wa, wb):
    n = ((np.asarray(wa, dtype=np.uint64) >> np.uint64(6)) << np.uint64(26)) + (np.asarray(wb, dtype=np.uint64) >> np.uint64(6))
    return (n.astype(np.float64) + 0.5) * 2.0 ** -52


def epi_log(x):
    """the library's logarithm (csrc/ekf_device.hpp) for finite x > 0"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    small = m < 0.70710678118654752440
    m = np.where(small, m + m, m)
    k = (e - small).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01))
    t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)))
    R = t2 + t1
    hfsq = 0.5 * f * f
    return k * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + k * 1.90821492927058770002e-10)) - f)


def _horner(c, r):
    acc = np.full_like(r, c[0])
    for v in c[1:]:
        acc = acc * r + v
    return acc


def icdf(u):
    u = np.asarray(u, dtype=np.float64)
    q = u - 0.5
    central = np.abs(q) <= 0.425
    r = 0.180625 - q * q
    zc = (_horner(A, r) * q) / _horner(B, r)
    rt = np.sqrt(-epi_log(np.where(q < 0.0, u, 1.0 - u)))
    near = rt <= 5.0
    r1, r2 = rt - 1.6, rt - 5.0
    x = np.where(near, _horner(CC, r1) / _horner(D, r1), _horner(E, r2) / _horner(F, r2))
    return np.where(central, zc, np.where(q < 0.0, -x, x))


def fill(seed, stream, t0, nt, rows, lane0, n_lanes):
    """out [nt, rows, n_lanes] float64: the window [t0, t0 + nt) x rows x [lane0, lane0 + n_lanes) of (seed, stream)"""
    seed, stream = int(seed), int(stream)
    lane = np.uint64(lane0) + np.arange(n_lanes, dtype=np.uint64)
    out = np.empty((nt, rows, n_lanes))
    for t in range(nt):
        tt = np.full(n_lanes, (int(t0) + t) & 0xFFFFFFFF, dtype=np.uint64)
        for q in range((rows + 1) // 2):
            c3 = np.full(n_lanes, 0x80000000 | (stream << 1) | q, dtype=np.uint64)
            w = philox(lane & M32, lane >> np.uint64(32), tt, c3, seed & 0xFFFFFFFF, seed >> 32)
            out[t, 2 * q] = icdf(uniform(w[0], w[1]))
            if 2 * q + 1 < rows:
                out[t, 2 * q + 1] = icdf(uniform(w[2], w[3]))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class NoiseRef:
    """tests/noise_ref.c as a shared object in build_dir"""

    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/noise_ref.c")
        so = os.path.join(str(build_dir), "libnoise_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.nzr_philox.argtypes = [C.c_void_p] * 3
        h.nzr_uniform.argtypes = [C.c_uint32] * 2
        h.nzr_icdf.argtypes = [C.c_double]
        h.nzr_uniform.restype = h.nzr_icdf.restype = C.c_double
        h.nzr_fill.argtypes = [C.c_uint32] * 4 + [C.c_int] * 2 + [C.c_uint64, C.c_int64, C.c_void_p]
        h.nzr_icdf_vec.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        h.nzr_philox.restype = h.nzr_fill.restype = h.nzr_icdf_vec.restype = None
        self.h = h

    def philox(self, ctr, key):
        c, k, o = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
        self.h.nzr_philox(c, k, o)
        return list(o)

    def uniform(self, wa, wb):
        return self.h.nzr_uniform(wa, wb)

    def icdf(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        z = np.empty_like(u)
        self.h.nzr_icdf_vec(u.size, u.ctypes.data, z.ctypes.data)
        return z

    def fill(self, seed, stream, t0, nt, rows, lane0, n_lanes):
        out = np.empty((nt, rows, n_lanes))
        seed = int(seed)
        self.h.nzr_fill(seed & 0xFFFFFFFF, seed >> 32, int(stream), int(t0), int(nt), int(rows), int(lane0), int(n_lanes), out.ctypes.data)
        return out
