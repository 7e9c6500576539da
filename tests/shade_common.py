"""Shared by tests/test_shade_rays_cpu.py and tests/test_shade_rays_gpu.py (test infrastructure): float-bit comparison, the rays
the shaded queries are tried with, the oracle's rayColor over many rays, and pixelColor (RK:91-98) restated in numpy float32."""
import ctypes
import os

import numpy as np

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- rays --------------------------------------------------------------------------------------------------------------------
def normalize_f32(d):
    """normalize() as the oracle fixes it: v / sqrt((x*x + y*y) + z*z), every operation a float32 operation."""
    d = np.asarray(d, F)
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return (d / ln[..., None]).astype(F)


def settled_unit(d):
    """-> unit vectors, and which rows of them normalize_f32 leaves bit for bit as they are.  One normalisation does not always
    give such a vector (the length of a normalised vector may round to 1 +- an ulp, and a few vectors go back and forth between two
    neighbours for ever); a 1x1 oracle frame normalises its `forwards` once more, so only settled rows can stand for their ray."""
    d = normalize_f32(d)
    for _ in range(4):
        d = normalize_f32(d)
    return d, (bits(normalize_f32(d)) == bits(d)).all(axis=-1)


def camera_rays(params, W, H):
    """The primary rays of a W x H frame (RK:76-86 in float32, the oracle's order) -> origins, directions, each (W * H, 3)."""
    p = np.asarray(params, F)
    cam, fw, rgt, up = p[0:3], p[4:7], p[8:11], p[12:15]
    ys, xs = np.mgrid[0:H, 0:W]
    xs = xs.reshape(-1); ys = ys.reshape(-1)
    hc = (xs.astype(F) - F(W) / F(2)) / F(W) * F(2)
    vc = (F(H) / F(2) - ys.astype(F)) / F(W) * F(2)
    d = np.stack([(fw[k] + hc * rgt[k]) + vc * up[k] for k in range(3)], axis=1).astype(F)
    return np.broadcast_to(cam, d.shape).astype(F), normalize_f32(d)


def random_rays(lo, hi, n, seed):
    """Incoherent rays: origins in the box grown by half its size on every side, directions of lengths 0.05 .. 20 (not unit)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    o = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.05, 20.0, (n, 1))
    return o, d.astype(F)


def axis_rays(lo, hi, seed, per_axis=100):
    """Directions along the axes (two components of the direction are zero)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (6 * per_axis, 3)).astype(F)
    d = np.zeros((6 * per_axis, 3), F)
    for k in range(6):
        d[k * per_axis:(k + 1) * per_axis, k // 2] = F(1.0 if k % 2 == 0 else -1.0) * F(0.5 + k)
    return o, d


def sphere_box(sp):
    sp = np.asarray(sp, F).reshape(-1, 8)
    return (sp[:, 0:3] - sp[:, 7:8]).min(axis=0), (sp[:, 0:3] + sp[:, 7:8]).max(axis=0)


def pack(o, d):
    rays = np.zeros((o.shape[0], 8), F)
    rays[:, 0:3], rays[:, 4:7] = o, d
    return rays


# ---- the oracle over many rays -------------------------------------------------------------------------------------------------
class _Face(ctypes.Structure):
    _fields_ = [("w", ctypes.c_uint32), ("h", ctypes.c_uint32), ("rgba", ctypes.c_void_p)]


class OracleRays:
    """rt_oracle_ray_color and rt_oracle_cube_sample for arrays of rays: one C call per ray, the arguments prepared once."""
    _lib = None

    def __init__(self, oracle, params, spheres, faces):
        oracle.lib()                                   # built if need be
        if OracleRays._lib is None:                    # a handle of our own: plain addresses as arguments
            L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), "librt_oracle.so"))
            vp = ctypes.c_void_p
            L.rt_oracle_ray_color.restype = None
            L.rt_oracle_ray_color.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
            L.rt_oracle_cube_sample.restype = None
            L.rt_oracle_cube_sample.argtypes = [vp, vp, vp]
            OracleRays._lib = L
        self.params = np.ascontiguousarray(params, dtype=F)
        self.spheres = np.ascontiguousarray(spheres, dtype=F).reshape(-1, 8)
        self.keep = [np.ascontiguousarray(f, dtype=np.uint8) for f in faces]
        self.faces = (_Face * 6)()
        for i, f in enumerate(self.keep):
            self.faces[i].w, self.faces[i].h, self.faces[i].rgba = f.shape[1], f.shape[0], f.ctypes.data

    def ray_color(self, o, d):
        """-> (n, 4) float32 {r, g, b, dist}, (n,) scene traversals of each path"""
        o = np.ascontiguousarray(o, dtype=F).reshape(-1, 3)
        d = np.ascontiguousarray(d, dtype=F).reshape(-1, 3)
        out = np.zeros((o.shape[0], 4), F)
        cnt = np.zeros(o.shape[0], np.uint64)
        fn, pa, sp, n = OracleRays._lib.rt_oracle_ray_color, self.params.ctypes.data, self.spheres.ctypes.data, self.spheres.shape[0]
        fa, po, pd, pr, pc = ctypes.addressof(self.faces), o.ctypes.data, d.ctypes.data, out.ctypes.data, cnt.ctypes.data
        for i in range(o.shape[0]):
            fn(pa, sp, n, fa, po + 12 * i, pd + 12 * i, pr + 16 * i, pc + 8 * i)
        return out, cnt

    def sky(self, d):
        """textureSampleLevel(skyTex, dir) -> (n, 3) float32"""
        d = np.ascontiguousarray(d, dtype=F).reshape(-1, 3)
        out = np.zeros((d.shape[0], 3), F)
        fn, fa, pd, pr = OracleRays._lib.rt_oracle_cube_sample, ctypes.addressof(self.faces), d.ctypes.data, out.ctypes.data
        for i in range(d.shape[0]):
            fn(fa, pd + 12 * i, pr + 12 * i)
        return out


# ---- RK:91-98 in numpy float32 -------------------------------------------------------------------------------------------------
def compose_np(rgbd, sky, min_intensity):
    """pixelColor (RK:91-96): k = clamp((30 - dist) / 30, 0, 1), k * rayColor + (1 - k) * (minIntensity * sky) -> (n, 3)"""
    rgbd, sky = np.asarray(rgbd, F), np.asarray(sky, F)
    with np.errstate(all="ignore"):
        k = np.fmin(np.fmax((F(30.0) - rgbd[:, 3]) / F(30.0), F(0.0)), F(1.0))[:, None]      # fmaxf / fminf, as clamp is fixed
        return (k * rgbd[:, 0:3] + (F(1.0) - k) * (F(min_intensity) * sky)).astype(F)


def quantise(rgb):
    """The rgba8unorm store (RK:98): floor(clamp(c, 0, 1) * 255 + 0.5), NaN -> 0 -> uint8"""
    c = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        q = np.floor(np.fmin(np.fmax(c, F(0.0)), F(1.0)) * F(255.0) + F(0.5))
    return np.where(np.isnan(c), F(0.0), q).astype(np.uint8)
