"""Poisson surface reconstruction of an oriented point cloud on the HIP path (csrc/poisson.hip; the contract is csrc/poisson.h, the
per-element rules csrc/poisson_math.h, restated by tests/poisson_oracle.py): the consumer of the normals ``cloud_clean`` produces.

The unscreened formulation (Kazhdan, Bolitho, Hoppe 2006) on a dense uniform grid with the layout of ``tsdf_mesh.TsdfVolume``:
the points' density W and their density-normalised normals V are splatted trilinearly (fixed point, integer atomics: two runs give
the same bits), Laplace chi = div V is solved with chi = 0 on the box by V(2,2) multigrid cycles (damped Jacobi, the wall imposed
through a mirrored ghost cell), the isovalue is the weighted mean of chi at the points, and the marching tetrahedra of
``TsdfVolume.extract`` read ``chi - iso`` as their signed distance.  Normals point outward, so chi rises outward, the inside is
negative and the faces point out.  ``trim`` cuts the surface where no sample is near: a voxel is observed when the largest density
in its 3 x 3 x 3 neighbourhood reaches ``trim``; 0 gives a watertight surface.

    python -m rc_mvsnet_amd.poisson_mesh --in cloud.ply --out mesh.ply --resolution 256 --trim-relative 0.05 --keep-largest 1

Limits: unscreened (no point-interpolation term, so smoother than screened Poisson at equal resolution); a dense grid of at most
2^27 voxels (512^3); trilinear splats, no per-point confidence; colours are a weighted mean, grey where no sample reached; an
elongated grid coarsens only while every side allows, so it converges more slowly (the residuals are in the stats).  No CPU fallback."""
import argparse
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib, fusion
from .mesh_clean import _ptr
from .tsdf_mesh import TsdfVolume, mesh_ply_bytes

MAX_VOXELS, MAX_LEVELS, MAX_CYCLES, ACC, COUNTERS, STATS, PART = (_lib.CONSTANTS["RCMVS_PO_" + k] for k in
                                                                  ("MAX_VOXELS", "MAX_LEVELS", "MAX_CYCLES", "ACC", "COUNTERS", "STATS", "PART"))
PHASES = {k.lower(): _lib.CONSTANTS["RCMVS_PO_PHASE_" + k] for k in ("ALL", "DENSITY", "NORMAL", "SWEEP", "RESTRICT", "PROLONG")}
MOMENT_BLOCKS = _lib.CONSTANTS["RCMVS_PC_MOMENT_BLOCKS"]
COUNTER_NAMES = ("splatted", "non_finite", "zero_normal", "outside")


def _call(name, args, _timed):
    if _timed is None:
        _lib.call(name, *args, fusion._stream())
    else:
        _lib.call(name + "_timed", *args, PHASES[_timed[0]], _timed[1], _timed[2], fusion._stream())


def level_dims(dims):
    """The multigrid levels of a grid, finest first: a level is coarsened by two while all its sides are even and the smallest
    coarser side is at least 4"""
    levels = [[int(d) for d in dims]]
    while len(levels) < MAX_LEVELS and all(d % 2 == 0 and d // 2 >= 4 for d in levels[-1]):
        levels.append([d // 2 for d in levels[-1]])
    return levels


def plan_grid(lo, hi, resolution=256, scale=1.25, multiple=16):
    """The box lo .. hi of the finite points -> (origin, voxel, dims): the box scaled about its centre, voxel = its longest side /
    resolution, every side rounded up to a multiple of ``multiple`` voxels, the box centred in the grid"""
    what = "poisson_mesh.plan_grid"
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise _lib.RcmvsError(f"{what}: box {lo.tolist()} .. {hi.tolist()} (finite, hi >= lo)")
    if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or resolution < 1:
        raise _lib.RcmvsError(f"{what}: resolution = {resolution!r} (an integer >= 1)")
    if isinstance(multiple, bool) or not isinstance(multiple, (int, np.integer)) or multiple < 1:
        raise _lib.RcmvsError(f"{what}: multiple = {multiple!r} (an integer >= 1)")
    if not (math.isfinite(scale) and scale >= 1.0):
        raise _lib.RcmvsError(f"{what}: scale = {scale!r} (finite and >= 1)")
    side = (hi - lo) * float(scale)
    longest = float(side.max())
    if not longest > 0:
        raise _lib.RcmvsError(f"{what}: the box has no extent")
    h = longest / int(resolution)
    dims = [max(int(multiple), int(multiple) * int(math.ceil(math.ceil(s / h - 1e-9) / multiple))) for s in side]
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise _lib.RcmvsError(f"{what}: {dims[0]} x {dims[1]} x {dims[2]} voxels (at most 2^27): lower the resolution")
    centre = 0.5 * (lo + hi)
    origin = [float(centre[a] - 0.5 * dims[a] * h) for a in range(3)]
    return origin, h, dims


class PoissonVolume:
    """A gx x gy x gz grid of cubic voxels of edge ``voxel`` with its lower corner at ``origin`` (the layout of TsdfVolume): splat() an
    oriented cloud, solve() the Poisson equation, field() the TsdfVolume whose extract() gives the surface.  ``stats`` collects what
    each step found."""

    def __init__(self, origin, voxel, dims, device):
        self.grid = [float(origin[0]), float(origin[1]), float(origin[2]), float(voxel)]
        self.dims = [int(d) for d in dims]
        if len(self.dims) != 3 or min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] > MAX_VOXELS:
            raise _lib.RcmvsError(f"PoissonVolume: dims {self.dims} (three sides >= 1, at most 2^27 voxels)")
        if not all(math.isfinite(v) for v in self.grid) or not self.grid[3] > 0:
            raise _lib.RcmvsError(f"PoissonVolume: origin {self.grid[:3]}, voxel {self.grid[3]} (finite, voxel positive)")
        self.voxels = self.dims[0] * self.dims[1] * self.dims[2]
        self.device = torch.device(device)
        self.levels = level_dims(self.dims)
        self.stats = {"levels": self.levels, "voxel": self.grid[3], "origin": self.grid[:3], "residual": []}
        self.xyz = self.point = self.acc = self.W = self.V = self.C = self.b = self.x = self.iso = None
        self._g = (ctypes.c_double * 4)(*self.grid)
        self._d = (ctypes.c_int * 3)(*self.dims)

    def _host(self):
        return ctypes.cast(self._g, ctypes.c_void_p), ctypes.cast(self._d, ctypes.c_void_p)

    def _plane(self):
        return torch.empty(self.voxels, device=self.device, dtype=torch.float32)

    def _need(self, have, what, first):
        if have is None:
            raise _lib.RcmvsError(f"PoissonVolume.{what}: {first}() comes first")

    def splat(self, xyz, normals, rgb=None, density_weight=True, _timed=None):
        """xyz (n,3) fp32, normals (n,3) fp32 (any length but 0), rgb (n,3) uint8 or None, on the volume's device: the density W,
        the vector field V, the colour means, and the right-hand side b = div V.  Points that are not finite, have a zero normal or
        do not have all eight voxels around them in the grid are skipped and counted."""
        what = "PoissonVolume.splat"
        for t, name in ((xyz, "xyz"), (normals, "normals")):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
                raise _lib.RcmvsError(f"{what}: {name} must be an (n,3) float32 tensor, got "
                                      f"{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}")
        n = int(xyz.shape[0])
        if int(normals.shape[0]) != n:
            raise _lib.RcmvsError(f"{what}: {n} points, {int(normals.shape[0])} normals")
        if n >= 1 << 31:
            raise _lib.RcmvsError(f"{what}: n = {n} points (below 2^31)")
        if rgb is not None and (not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (n, 3)):
            raise _lib.RcmvsError(f"{what}: rgb must be an ({n},3) uint8 tensor or None")
        dev = self.device
        colour = rgb is not None
        self.acc = torch.empty((ACC if colour else 4) * self.voxels, device=dev, dtype=torch.int64)
        self.W, self.V = self._plane(), [self._plane() for _ in range(3)]
        self.C = [self._plane() for _ in range(3)] if colour else None
        self.point = torch.empty((n, 2), device=dev, dtype=torch.float64)
        counters = torch.empty(COUNTERS, device=dev, dtype=torch.int64)
        self.xyz = xyz
        cp = [_ptr(None if self.C is None else self.C[c], "C", torch.float32) for c in range(3)]
        _call("rcmvs_po_splat", [_ptr(xyz, "xyz", torch.float32), _ptr(normals, "normals", torch.float32), _ptr(rgb, "rgb", torch.uint8), n,
                                 1 if density_weight else 0, *self._host(), fusion._chk(self.acc, "acc", torch.int64), fusion._chk(self.W, "W"),
                                 *[fusion._chk(v, "V") for v in self.V], *cp, _ptr(self.point, "point", torch.float64),
                                 fusion._chk(counters, "counters", torch.int64)], _timed)
        self.b = self._plane()
        _call("rcmvs_po_rhs", [*[fusion._chk(v, "V") for v in self.V], *self._host(), fusion._chk(self.b, "b")], None)
        self.x, self.iso = None, None
        self.stats.update({"points": n, "density_weight": bool(density_weight), "colour": colour, "residual": [],
                           **dict(zip(COUNTER_NAMES, (int(c) for c in counters.cpu().tolist())))})
        return self

    def coarse_floats(self):
        return 3 * sum(math.prod(d) for d in self.levels[1:])

    def solve(self, cycles=8, _timed=None):
        """``cycles`` more V(2,2) cycles on chi (which starts at 0); the max-norm residual after each joins stats["residual"].
        Nothing is read back inside the loop; the residuals are read once at the end."""
        what = "PoissonVolume.solve"
        self._need(self.b, "solve", "splat")
        if isinstance(cycles, bool) or not isinstance(cycles, (int, np.integer)) or not 0 <= cycles <= MAX_CYCLES:
            raise _lib.RcmvsError(f"{what}: cycles = {cycles!r} (an integer, 0 .. {MAX_CYCLES})")
        cycles, dev = int(cycles), self.device
        if self.x is None:
            self.x = torch.zeros(self.voxels, device=dev, dtype=torch.float32)
            self._tmp = self._plane()
            self.coarse = torch.empty(self.coarse_floats(), device=dev, dtype=torch.float32)
            self._part = torch.empty(PART, device=dev, dtype=torch.float64)
        resid = torch.empty(cycles, device=dev, dtype=torch.float64)
        _call("rcmvs_po_solve", [fusion._chk(self.x, "x"), fusion._chk(self._tmp, "tmp"), fusion._chk(self.b, "b"), _ptr(self.coarse, "coarse", torch.float32),
                                 *self._host(), cycles, fusion._chk(self._part, "part", torch.float64), _ptr(resid, "resid", torch.float64)], _timed)
        self.stats["residual"] += resid.cpu().tolist()
        self.iso = None
        return self

    def isovalue(self, _timed=None):
        """-> the (STATS,) fp64 device tensor {iso, sum s chi, sum s, sum W_p, splatted, mean W_p, min W_p, 0}; joins the stats"""
        self._need(self.x, "isovalue", "solve")
        n, dev = int(self.xyz.shape[0]), self.device
        terms = torch.empty(4 * n, device=dev, dtype=torch.float64)
        part = torch.empty(5 * MOMENT_BLOCKS, device=dev, dtype=torch.float64)
        self.iso = torch.empty(STATS, device=dev, dtype=torch.float64)
        _call("rcmvs_po_iso", [_ptr(self.xyz, "xyz", torch.float32), _ptr(self.point, "point", torch.float64), n, fusion._chk(self.x, "chi"), *self._host(),
                               _ptr(terms, "terms", torch.float64), fusion._chk(part, "part", torch.float64), fusion._chk(self.iso, "stats", torch.float64)], _timed)
        s = self.iso.cpu().tolist()
        self.stats.update({"iso": s[0], "wp_mean": s[5], "wp_min": s[6] if s[4] > 0 else None})
        return self.iso

    def field(self, trim=0.0, trim_relative=None, _timed=None):
        """-> the TsdfVolume of chi - iso (extract() it with min_weight = 1): a voxel is observed where the largest density of its
        3 x 3 x 3 neighbourhood is >= trim.  trim_relative = f: trim = f times the mean of W_p over the splatted points."""
        what = "PoissonVolume.field"
        self._need(self.x, "field", "solve")
        if self.iso is None:
            self.isovalue()
        if trim_relative is not None:
            f = float(trim_relative)
            if not (math.isfinite(f) and f >= 0):
                raise _lib.RcmvsError(f"{what}: trim_relative = {trim_relative!r} (finite and >= 0)")
            trim = f * self.stats["wp_mean"]
        try:
            trim = float(trim)
        except (TypeError, ValueError):
            raise _lib.RcmvsError(f"{what}: trim = {trim!r} (a number >= 0)") from None
        if not (math.isfinite(trim) and trim >= 0):
            raise _lib.RcmvsError(f"{what}: trim = {trim!r} (finite and >= 0)")
        vol = TsdfVolume(self.grid[:3], self.grid[3], self.dims, self.device, colour=False)
        vol.dsum, vol.wsum = self._plane(), self._plane()
        vol.csum = self.C
        trimmed = torch.empty(1, device=self.device, dtype=torch.int64)
        _call("rcmvs_po_field", [fusion._chk(self.x, "chi"), fusion._chk(self.W, "W"), fusion._chk(self.iso, "stats", torch.float64), trim, self._host()[1],
                                 fusion._chk(vol.dsum, "dsum"), fusion._chk(vol.wsum, "wsum"), fusion._chk(trimmed, "trimmed", torch.int64)], _timed)
        self.stats.update({"trim": trim, "trimmed_voxels": int(trimmed.item())})
        return vol


def _bounds(xyz, normals):
    """the box of the points with finite coordinates and normals (host: six numbers)"""
    ok = torch.isfinite(xyz).all(dim=1) & torch.isfinite(normals).all(dim=1)
    if not bool(ok.any()):
        raise _lib.RcmvsError("poisson_mesh.reconstruct: no point with finite coordinates and normal")
    p = xyz[ok]
    return p.min(dim=0).values.cpu().numpy().astype(np.float64), p.max(dim=0).values.cpu().numpy().astype(np.float64)


def reconstruct(xyz, normals, rgb=None, resolution=256, scale=1.25, cycles=8, trim=0.0, trim_relative=None, clean=None, density_weight=True, grid=None):
    """xyz, normals (n,3) fp32, rgb (n,3) uint8 or None on the device -> (verts (nv,3) fp32, faces (nf,3) int32, rgb (nv,3) uint8 or
    None, stats).  The grid is plan_grid's over the finite points (``grid`` = (origin, voxel, dims) overrides it); ``clean``: the
    keyword arguments of mesh_clean.clean_mesh (``{"keep_largest": 1}`` keeps the largest surface), whose stats join as "clean"."""
    if not torch.is_tensor(xyz) or not torch.is_tensor(normals) or xyz.dim() != 2 or normals.shape != xyz.shape:
        raise _lib.RcmvsError("poisson_mesh.reconstruct: xyz and normals must be (n,3) float32 tensors of one length")
    if grid is None:
        lo, hi = _bounds(xyz, normals)
        grid = plan_grid(lo, hi, resolution, scale)
    vol = PoissonVolume(*grid, xyz.device)
    vol.splat(xyz, normals, rgb, density_weight).solve(cycles)
    verts, faces, col = vol.field(trim, trim_relative).extract(1)
    stats = dict(vol.stats)
    if clean is not None:
        from . import mesh_clean
        verts, faces, col, stats["clean"] = mesh_clean.clean_mesh(verts, faces, col, **clean)
    stats.update({"vertices": int(verts.shape[0]), "faces": int(faces.shape[0])})
    return verts, faces, col, stats


def poisson_options(enabled=False, resolution=256, trim_relative=None, cycles=8):
    """The drivers' options (--poisson, --poisson-resolution, --poisson-trim-relative, --poisson-cycles) -> the keyword arguments of
    reconstruct, or None without --poisson"""
    if not enabled:
        return None
    return {"resolution": int(resolution), "trim_relative": None if trim_relative is None else float(trim_relative), "cycles": int(cycles)}


def main(argv=None):
    from . import dtu_io, mesh_clean, mesh_normals
    ap = argparse.ArgumentParser(description="Poisson surface reconstruction of a point-cloud PLY with normals")
    ap.add_argument("--in", dest="src", required=True, help="the PLY to read: positions, nx ny nz, vertex colours when it has them")
    ap.add_argument("--out", required=True, help="the mesh PLY to write")
    ap.add_argument("--resolution", type=int, default=256, help="voxels along the longest side of the scaled box")
    ap.add_argument("--scale", type=float, default=1.25, help="the box of the points is scaled by this about its centre")
    ap.add_argument("--cycles", type=int, default=8, help="V(2,2) multigrid cycles")
    trims = ap.add_mutually_exclusive_group()
    trims.add_argument("--trim", type=float, default=0.0, help="cut the surface where the dilated density is below T (0: watertight)")
    trims.add_argument("--trim-relative", type=float, default=None, metavar="F", help="T = F times the mean density at the points")
    ap.add_argument("--no-density-weight", action="store_true", help="splat the normals as they are, without 1 / density")
    ap.add_argument("--keep-largest", type=int, default=0, metavar="K", help="keep only the K components with most faces")
    ap.add_argument("--min-faces", type=int, default=0, metavar="N", help="drop components with fewer faces")
    ap.add_argument("--normals", choices=("area", "sphere"), default=None, help="add per-vertex normals to the mesh")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    xyz, rgb, nrm = dtu_io.read_ply_cloud_normals(a.src)
    if nrm is None:
        ap.error(f"{a.src} has no normals (nx ny nz): add them with `python -m rc_mvsnet_amd.cloud_clean --normals K`")
    dev = torch.device(a.device)
    verts, faces, col, stats = reconstruct(torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev),
                                           torch.from_numpy(np.ascontiguousarray(nrm, np.float32)).to(dev),
                                           None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).to(dev),
                                           resolution=a.resolution, scale=a.scale, cycles=a.cycles, trim=a.trim, trim_relative=a.trim_relative,
                                           clean=mesh_clean.clean_options(min_faces=a.min_faces, keep_largest=a.keep_largest),
                                           density_weight=not a.no_density_weight)
    vn = None
    if a.normals:
        vn, stats["normals"] = mesh_normals.vertex_normals(verts, faces, a.normals)
    with open(a.out, "wb") as f:
        f.write(mesh_ply_bytes(verts, faces, col, vn))
    summary = {"in": a.src, "out": a.out, "poisson": stats}
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
