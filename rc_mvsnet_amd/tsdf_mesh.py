"""Depth maps -> triangle mesh on the HIP path: TSDF fusion into a dense voxel grid and marching tetrahedra
(csrc/tsdf_mesh.hip; the contract is csrc/tsdf_mesh.h, the arithmetic csrc/tsdf_mesh_math.h, restated by tests/tsdf_oracle.py).

``TsdfVolume`` holds the planar fp32 state on the device; ``integrate`` adds views sixteen to a launch (a voxel's state is read
and written once per launch, and the result does not depend on the chunking), ``extract`` runs count / scan / emit and returns
vertices, faces and vertex colours as device tensors.  ``mesh_scan`` is the mesh counterpart of ``fusion.filter_depth``: the same
``fusion.fuse_view`` per reference view, its filtered ``depth_avg`` integrated instead of back-projected, one PLY written.

    python -m rc_mvsnet_amd.tsdf_mesh --pair-folder data/scan9 --scan-folder out/scan9 --out-folder out/scan9 --mesh out/scan9_mesh.ply

``SparseTsdfVolume`` (csrc/tsdf_sparse.hip, contract csrc/tsdf_sparse.h) is the volume of a large scene: 8 x 8 x 8-voxel blocks
allocated only where the truncation slab of a depth pixel passes (mark, build), then the same integrate / extract per allocated
voxel.  With no skipped pixel its mesh is the dense mesh of the same grid in another order.  ``mesh_scan(sparse=True)``, ``--sparse``
and ``mesh_scan_tanks`` use it.

Limits: both volumes are axis-aligned.  The dense grid has at most 2^28 voxels; the sparse one at most 2^27 blocks (4096^3 voxels) of
which at most 2^19 are active, its block set does not grow after build(), and a pixel whose slab spans more than 4 blocks on an
axis is skipped and counted (with any skipped pixel the equality with the dense mesh is no longer guaranteed).  Hole filling is
rc_mvsnet_amd.mesh_holes' (``fill_holes``), decimation rc_mvsnet_amd.mesh_decimate's (``decimate_cell`` / ``decimate_voxels``); marching tetrahedra emits roughly twice the
triangles of marching cubes; as extracted, the mesh carries floating
fragments and vertices at the rim of the observed region that no face uses.  No CPU fallback.

``min_faces`` / ``min_fraction`` / ``keep_largest`` / ``smooth`` / ``fill_holes`` (``--min-faces`` ...) run rc_mvsnet_amd.mesh_clean.clean_mesh
between the extraction and the write: small components and unreferenced vertices removed, boundary loops of at most ``fill_holes``
edges closed, Taubin smoothing.  With none of them given
nothing of it runs and the PLY and the summary are what they were.

``render_dir`` (``--render DIR``) renders the mesh just written into the views it was fused from (rc_mvsnet_amd.mesh_render), writes
their depth PFMs and shade / colour PNGs under that folder, compares the rendered depth with the filtered depth maps still on the
device and adds the summed table to the summary as "render".  Without it nothing of it runs.

``normals`` (``--normals area|sphere``) computes oriented per-vertex normals of the final mesh (rc_mvsnet_amd.mesh_normals), after
the clean-up and the decimation: the PLY's vertex records become x y z nx ny nz red green blue, the summary gains the counters as
"normals", and a render gains the smooth shade and the normal image.  Without it nothing of it runs and the PLY bytes are what
they were.

``texture`` (``--texture [--texture-size N]``) textures the final mesh from the images and cameras of the views it was fused from
(rc_mvsnet_amd.mesh_texture), last of all: the PLY's faces gain six texture coordinates each and the header names the atlas, which is
written next to the PLY as <name>.png; the summary gains the counters and the atlas size as "texture", and a render gains the
textured views.  Without it nothing of it runs and the PLY bytes are what they were."""
import argparse
import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib, fusion, mesh_clean, mesh_decimate, scan_io
from .data_io import read_pfm

MAX_VOXELS, MAX_VIEWS, SCAN_TILE = (_lib.CONSTANTS[k] for k in ("RCMVS_TSDF_MAX_VOXELS", "RCMVS_TSDF_MAX_VIEWS", "RCMVS_TSDF_SCAN_TILE"))
SP_BLOCK, SP_MAX_BLOCKS, SP_MAX_ACTIVE, SP_SCAN_TILE = (_lib.CONSTANTS["RCMVS_TSDF_SP_" + k] for k in ("BLOCK", "MAX_BLOCKS", "MAX_ACTIVE", "SCAN_TILE"))
SP_VOXELS = SP_BLOCK ** 3
_NULL = ctypes.c_void_p(0)


def _ptr(t, name, dtype):
    return _NULL if t is None else fusion._chk(t, name, dtype)


class TsdfVolume:
    """A gx x gy x gz grid of cubic voxels of edge ``voxel`` with its lower corner at ``origin``; voxel (i, j, k) is number
    i + gx * (j + gy * k) and has its centre at origin + (idx + 0.5) * voxel."""

    def __init__(self, origin, voxel, dims, device, colour=True):
        self.grid = [float(origin[0]), float(origin[1]), float(origin[2]), float(voxel)]
        self.dims = [int(d) for d in dims]
        if len(self.dims) != 3 or min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] > MAX_VOXELS:
            raise _lib.RcmvsError(f"TsdfVolume: dims {self.dims} (three sides >= 1, at most 2^28 voxels)")
        if not all(math.isfinite(v) for v in self.grid) or not self.grid[3] > 0:
            raise _lib.RcmvsError(f"TsdfVolume: origin {self.grid[:3]}, voxel {self.grid[3]} (finite, voxel positive)")
        self.voxels = self.dims[0] * self.dims[1] * self.dims[2]
        self.device = torch.device(device)
        self.dsum = torch.zeros(self.voxels, device=self.device, dtype=torch.float32)
        self.wsum = torch.zeros(self.voxels, device=self.device, dtype=torch.float32)
        self.csum = [torch.zeros(self.voxels, device=self.device, dtype=torch.float32) for _ in range(3)] if colour else None

    def _host(self):
        return (ctypes.c_double * 4)(*self.grid), (ctypes.c_int * 3)(*self.dims)

    def _colour_ptrs(self):
        return [_ptr(None if self.csum is None else self.csum[c], "csum", torch.float32) for c in range(3)]

    def integrate(self, depth, cams, rgb=None, trunc=None):
        """depth (n,H,W) fp32 and rgb (n,H,W,3) uint8 (or None) on the device, cams (n,16) {R row-major 9, t 3, fx, fy, cx, cy}
        world -> camera on the host; any n, sixteen views to a launch."""
        if trunc is None:
            raise _lib.RcmvsError("TsdfVolume.integrate: trunc (the truncation distance, in world units) is required")
        if depth.dim() != 3:
            raise _lib.RcmvsError(f"TsdfVolume.integrate: expected (n,H,W) depth maps, got {tuple(depth.shape)}")
        n, H, W = (int(s) for s in depth.shape)
        cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float64).reshape(-1, 16))
        if len(cams) != n or (rgb is not None and tuple(rgb.shape) != (n, H, W, 3)):
            raise _lib.RcmvsError(f"TsdfVolume.integrate: {n} depth maps of {H} x {W}, {len(cams)} cameras, rgb {None if rgb is None else tuple(rgb.shape)}")
        grid, dims = self._host()
        for lo in range(0, n, MAX_VIEWS):
            hi = min(lo + MAX_VIEWS, n)
            _lib.call("rcmvs_tsdf_integrate", fusion._chk(depth[lo:hi], "depth"), _ptr(None if rgb is None else rgb[lo:hi], "rgb", torch.uint8),
                      hi - lo, H, W, cams[lo:hi].ctypes.data_as(ctypes.c_void_p), float(trunc), grid, dims, fusion._chk(self.dsum, "dsum"),
                      fusion._chk(self.wsum, "wsum"), *self._colour_ptrs(), fusion._stream())
        return self

    def count(self, min_weight=1):
        """-> (edge_mask, tri_count (uint8 per voxel), vert_start, tri_start (voxels + 1 int32), (vertices, faces) as ints)"""
        dev, n = self.device, self.voxels
        edge_mask = torch.empty(n, device=dev, dtype=torch.uint8)
        tri_count = torch.empty(n, device=dev, dtype=torch.uint8)
        work = torch.empty(256 + 2 * ((n + SCAN_TILE - 1) // SCAN_TILE), device=dev, dtype=torch.int32)
        vert_start = torch.empty(n + 1, device=dev, dtype=torch.int32)
        tri_start = torch.empty(n + 1, device=dev, dtype=torch.int32)
        totals = torch.empty(2, device=dev, dtype=torch.int64)
        _lib.call("rcmvs_tsdf_mesh_count", fusion._chk(self.dsum, "dsum"), fusion._chk(self.wsum, "wsum"), self._host()[1], int(min_weight),
                  fusion._chk(edge_mask, "edge_mask", torch.uint8), fusion._chk(tri_count, "tri_count", torch.uint8),
                  fusion._chk(work, "scan_work", torch.int32), fusion._chk(vert_start, "vert_start", torch.int32),
                  fusion._chk(tri_start, "tri_start", torch.int32), fusion._chk(totals, "totals", torch.int64), fusion._stream())
        nv, nf = (int(t) for t in totals.cpu())                      # the one host synchronisation of an extraction
        return edge_mask, tri_count, vert_start, tri_start, (nv, nf)

    def extract(self, min_weight=1):
        """-> (verts (nv,3) fp32, faces (nf,3) int32, rgb (nv,3) uint8 or None without colour planes), device tensors"""
        edge_mask, tri_count, vert_start, tri_start, (nv, nf) = self.count(min_weight)
        if nv >= 1 << 31 or nf >= 1 << 31:
            raise _lib.RcmvsError(f"TsdfVolume.extract: {nv} vertices, {nf} faces (below 2^31 each): use larger voxels")
        dev = self.device
        verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
        rgb = torch.empty((nv, 3), device=dev, dtype=torch.uint8) if self.csum is not None else None
        grid, dims = self._host()
        _lib.call("rcmvs_tsdf_mesh_emit", fusion._chk(self.dsum, "dsum"), fusion._chk(self.wsum, "wsum"), *self._colour_ptrs(), grid, dims,
                  int(min_weight), fusion._chk(edge_mask, "edge_mask", torch.uint8), fusion._chk(tri_count, "tri_count", torch.uint8),
                  fusion._chk(vert_start, "vert_start", torch.int32), fusion._chk(tri_start, "tri_start", torch.int32), nv, nf,
                  _ptr(verts if nv else None, "verts", torch.float32), _ptr(rgb if nv else None, "vert_rgb", torch.uint8),
                  _ptr(faces if nf else None, "faces", torch.int32), fusion._stream())
        return verts, faces, rgb


class SparseTsdfVolume:
    """A virtual grid of bx x by x bz blocks of 8 x 8 x 8 voxels of which only the marked blocks are allocated (csrc/tsdf_sparse.h).
    The order is mark (any number of times; ``flags`` may also be written directly), build, integrate, count / extract; the block set
    does not grow after build.  A voxel's planes equal TsdfVolume's planes of the same voxel in a grid of 8 * bdims voxels."""

    def __init__(self, origin, voxel, bdims, device, colour=True):
        self.grid = [float(origin[0]), float(origin[1]), float(origin[2]), float(voxel)]
        self.bdims = [int(d) for d in bdims]
        if len(self.bdims) != 3 or min(self.bdims) < 1 or self.bdims[0] * self.bdims[1] * self.bdims[2] > SP_MAX_BLOCKS:
            raise _lib.RcmvsError(f"SparseTsdfVolume: bdims {self.bdims} (three sides >= 1, at most 2^27 blocks)")
        if not all(math.isfinite(v) for v in self.grid) or not self.grid[3] > 0:
            raise _lib.RcmvsError(f"SparseTsdfVolume: origin {self.grid[:3]}, voxel {self.grid[3]} (finite, voxel positive)")
        self.blocks = self.bdims[0] * self.bdims[1] * self.bdims[2]
        self.dims = [SP_BLOCK * b for b in self.bdims]
        self.device = torch.device(device)
        self.colour = bool(colour)
        self.flags = torch.zeros(self.blocks, device=self.device, dtype=torch.uint8)
        self._skipped = torch.zeros(1, device=self.device, dtype=torch.int64)
        self.n_active = None                                        # set by build()

    def _host(self):
        return (ctypes.c_double * 4)(*self.grid), (ctypes.c_int * 3)(*self.bdims)

    def _need(self, built, what):
        if built != (self.n_active is not None):
            raise _lib.RcmvsError(f"SparseTsdfVolume.{what}: " + ("call build() first" if built else "the block set is fixed by build()"))

    def _colour_ptrs(self):
        return [_ptr(None if self.csum is None else self.csum[c], "csum", torch.float32) for c in range(3)]

    def _table(self):
        return (fusion._chk(self.mask_words, "mask_words", torch.int32), fusion._chk(self.word_rank, "word_rank", torch.int32),
                fusion._chk(self.active, "active", torch.int32), self.n_active)

    @staticmethod
    def _views(depth, cams, rgb, what):
        if depth.dim() != 3:
            raise _lib.RcmvsError(f"SparseTsdfVolume.{what}: expected (n,H,W) depth maps, got {tuple(depth.shape)}")
        n, H, W = (int(s) for s in depth.shape)
        cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float64).reshape(-1, 16))
        if len(cams) != n or (rgb is not None and tuple(rgb.shape) != (n, H, W, 3)):
            raise _lib.RcmvsError(f"SparseTsdfVolume.{what}: {n} depth maps of {H} x {W}, {len(cams)} cameras, rgb {None if rgb is None else tuple(rgb.shape)}")
        return n, H, W, cams

    def mark(self, depth, cams, trunc):
        """Flags the blocks that the truncation slabs of the depth pixels touch: depth (n,H,W) fp32 on the device, cams (n,16) on the
        host as for integrate; any n, sixteen views to a launch."""
        self._need(False, "mark")
        n, H, W, cams = self._views(depth, cams, None, "mark")
        grid, bdims = self._host()
        for lo in range(0, n, MAX_VIEWS):
            hi = min(lo + MAX_VIEWS, n)
            _lib.call("rcmvs_tsdf_sp_mark", fusion._chk(depth[lo:hi], "depth"), hi - lo, H, W, cams[lo:hi].ctypes.data_as(ctypes.c_void_p), float(trunc),
                      grid, bdims, fusion._chk(self.flags, "flags", torch.uint8), fusion._chk(self._skipped, "skipped", torch.int64), fusion._stream())
        return self

    def build(self):
        """Fixes the block set from ``flags`` and allocates the planes -> the number of active blocks."""
        self._need(False, "build")
        dev, words = self.device, (self.blocks + 31) // 32
        self.mask_words = torch.empty(words, device=dev, dtype=torch.int32)
        self.word_rank = torch.empty(words + 1, device=dev, dtype=torch.int32)
        active = torch.empty(min(self.blocks, SP_MAX_ACTIVE), device=dev, dtype=torch.int32)
        work = torch.empty((words + SP_SCAN_TILE - 1) // SP_SCAN_TILE, device=dev, dtype=torch.int32)
        _lib.call("rcmvs_tsdf_sp_build", fusion._chk(self.flags, "flags", torch.uint8), self._host()[1], fusion._chk(self.mask_words, "mask_words", torch.int32),
                  fusion._chk(self.word_rank, "word_rank", torch.int32), fusion._chk(active, "active", torch.int32), int(active.numel()),
                  fusion._chk(work, "scan_work", torch.int32), fusion._stream())
        total = int(self.word_rank[words:].cpu()[0]) & 0xffffffff      # the one host synchronisation of a build
        self.skipped = int(self._skipped.cpu()[0])
        if total < 1 or total > SP_MAX_ACTIVE:
            raise _lib.RcmvsError(f"SparseTsdfVolume.build: {total} active blocks of {self.blocks} (1 .. 2^19): " +
                                  ("no depth sample falls into the grid" if total < 1 else "use larger voxels or tighter bounds"))
        self.active = active[:total].contiguous()
        self.n_active, self.voxels = total, total * SP_VOXELS
        self.dsum = torch.zeros(self.voxels, device=dev, dtype=torch.float32)
        self.wsum = torch.zeros(self.voxels, device=dev, dtype=torch.float32)
        self.csum = [torch.zeros(self.voxels, device=dev, dtype=torch.float32) for _ in range(3)] if self.colour else None
        return total

    def integrate(self, depth, cams, rgb=None, trunc=None):
        """As TsdfVolume.integrate, on the allocated voxels."""
        self._need(True, "integrate")
        if trunc is None:
            raise _lib.RcmvsError("SparseTsdfVolume.integrate: trunc (the truncation distance, in world units) is required")
        n, H, W, cams = self._views(depth, cams, rgb, "integrate")
        grid, bdims = self._host()
        for lo in range(0, n, MAX_VIEWS):
            hi = min(lo + MAX_VIEWS, n)
            _lib.call("rcmvs_tsdf_sp_integrate", fusion._chk(depth[lo:hi], "depth"), _ptr(None if rgb is None else rgb[lo:hi], "rgb", torch.uint8),
                      hi - lo, H, W, cams[lo:hi].ctypes.data_as(ctypes.c_void_p), float(trunc), grid, bdims, fusion._chk(self.active, "active", torch.int32),
                      self.n_active, fusion._chk(self.dsum, "dsum"), fusion._chk(self.wsum, "wsum"), *self._colour_ptrs(), fusion._stream())
        return self

    def count(self, min_weight=1):
        """-> (edge_mask, tri_count (uint8 per allocated voxel), vert_start, tri_start (voxels + 1 int32), (vertices, faces) as ints)"""
        self._need(True, "count")
        dev, n = self.device, self.voxels
        edge_mask = torch.empty(n, device=dev, dtype=torch.uint8)
        tri_count = torch.empty(n, device=dev, dtype=torch.uint8)
        work = torch.empty(1024 + 2 * self.n_active, device=dev, dtype=torch.int32)
        vert_start = torch.empty(n + 1, device=dev, dtype=torch.int32)
        tri_start = torch.empty(n + 1, device=dev, dtype=torch.int32)
        totals = torch.empty(2, device=dev, dtype=torch.int64)
        _lib.call("rcmvs_tsdf_sp_mesh_count", fusion._chk(self.dsum, "dsum"), fusion._chk(self.wsum, "wsum"), self._host()[1], *self._table(),
                  int(min_weight), fusion._chk(edge_mask, "edge_mask", torch.uint8), fusion._chk(tri_count, "tri_count", torch.uint8),
                  fusion._chk(work, "scan_work", torch.int32), fusion._chk(vert_start, "vert_start", torch.int32),
                  fusion._chk(tri_start, "tri_start", torch.int32), fusion._chk(totals, "totals", torch.int64), fusion._stream())
        nv, nf = (int(t) for t in totals.cpu())                      # the one host synchronisation of an extraction
        return edge_mask, tri_count, vert_start, tri_start, (nv, nf)

    def extract(self, min_weight=1):
        """-> (verts (nv,3) fp32, faces (nf,3) int32, rgb (nv,3) uint8 or None without colour planes), device tensors, ordered by
        the allocated voxel number"""
        edge_mask, tri_count, vert_start, tri_start, (nv, nf) = self.count(min_weight)
        if nv >= 1 << 31 or nf >= 1 << 31:
            raise _lib.RcmvsError(f"SparseTsdfVolume.extract: {nv} vertices, {nf} faces (below 2^31 each): use larger voxels")
        dev = self.device
        verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
        rgb = torch.empty((nv, 3), device=dev, dtype=torch.uint8) if self.csum is not None else None
        grid, bdims = self._host()
        _lib.call("rcmvs_tsdf_sp_mesh_emit", fusion._chk(self.dsum, "dsum"), fusion._chk(self.wsum, "wsum"), *self._colour_ptrs(), grid, bdims,
                  *self._table(), int(min_weight), fusion._chk(edge_mask, "edge_mask", torch.uint8), fusion._chk(tri_count, "tri_count", torch.uint8),
                  fusion._chk(vert_start, "vert_start", torch.int32), fusion._chk(tri_start, "tri_start", torch.int32), nv, nf,
                  _ptr(verts if nv else None, "verts", torch.float32), _ptr(rgb if nv else None, "vert_rgb", torch.uint8),
                  _ptr(faces if nf else None, "faces", torch.int32), fusion._stream())
        return verts, faces, rgb


def mesh_ply_bytes(verts, faces, rgb=None, normals=None, texcoords=None, texture_file=None):
    """Binary little-endian PLY of a triangle mesh: vertex properties x y z (float) red green blue (uchar), then ``element face``
    with ``property list uchar int vertex_indices``.  rgb None: white.  normals (nv,3) fp32: the vertex record is x y z nx ny nz
    (float) red green blue; without them the bytes are what they always were.  dtu_io.read_ply_mesh reads it back exactly, with
    or without normals; dtu_io.read_ply_mesh_normals returns them too.  texcoords (nf,3,2) fp32 (mesh_texture's "uv"): the header gains
    ``comment TextureFile <texture_file>`` and the face element a second property ``property list uchar float texcoord`` with the six
    floats u v of the corners a, b, c, the convention MeshLab reads; dtu_io.read_ply_mesh_texture returns them."""
    verts, faces = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (verts, faces))
    rgb = None if rgb is None else (rgb.cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb))
    normals = None if normals is None else (normals.cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals))
    nv, nf = len(verts), len(faces)
    if normals is not None and (normals.dtype != np.float32 or normals.shape != (nv, 3)):
        raise _lib.RcmvsError(f"mesh_ply_bytes: normals must be ({nv},3) float32")
    if texcoords is not None:
        texcoords = np.asarray(texcoords)
        if texcoords.dtype != np.float32 or texcoords.shape != (nf, 3, 2):
            raise _lib.RcmvsError(f"mesh_ply_bytes: texcoords must be ({nf},3,2) float32")
        if not isinstance(texture_file, str) or not texture_file or any(ch.isspace() or not ch.isascii() for ch in texture_file):
            raise _lib.RcmvsError(f"mesh_ply_bytes: texture_file = {texture_file!r} (the atlas's file name, ASCII without spaces, goes with texcoords)")
    elif texture_file is not None:
        raise _lib.RcmvsError("mesh_ply_bytes: texture_file without texcoords")
    extra = "" if normals is None else "property float nx\nproperty float ny\nproperty float nz\n"
    comment = "" if texcoords is None else "comment TextureFile %s\n" % texture_file
    fextra = "" if texcoords is None else "property list uchar float texcoord\n"
    head = ("ply\nformat binary_little_endian 1.0\n%selement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\n%s"
            "end_header\n" % (comment, nv, extra, nf, fextra)).encode("ascii")
    vrec = np.empty(nv, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([] if normals is None else [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]) +
                    [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, k in enumerate(("x", "y", "z")):
        vrec[k] = verts[:, i] if nv else 0
    if normals is not None:
        for i, k in enumerate(("nx", "ny", "nz")):
            vrec[k] = normals[:, i] if nv else 0
    for i, k in enumerate(("red", "green", "blue")):
        vrec[k] = 255 if rgb is None else rgb[:, i]
    frec = np.empty(nf, dtype=[("n", "u1"), ("v", "<i4", (3,))] + ([] if texcoords is None else [("m", "u1"), ("t", "<f4", (6,))]))
    frec["n"] = 3
    frec["v"] = faces.reshape(nf, 3)
    if texcoords is not None:
        frec["m"] = 6
        frec["t"] = texcoords.reshape(nf, 6)
    return head + vrec.tobytes() + frec.tobytes()


def camera_row(K, E):
    """(3,3) intrinsics and (4,4) world -> camera extrinsics -> the 16 doubles of rcmvs_tsdf_integrate"""
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    return np.concatenate([E[:3, :3].ravel(), E[:3, 3], [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]])


def _add_view(r, cam, depths, colours, rows, lo, hi):
    """one fuse_view result -> its depth_avg under the final mask, colours and camera row appended; -> the grown bounding box"""
    keep = r["masks"][2] != 0
    depths.append(torch.where(keep, r["depth_avg"], torch.zeros_like(r["depth_avg"])))
    colours.append(r["rgb"])
    rows.append(camera_row(*cam))
    if bool(keep.any()):
        pts = r["xyz"][keep].double()
        pts = pts[torch.isfinite(pts).all(1)]
        if len(pts):
            a, b = pts.min(0).values.cpu().numpy(), pts.max(0).values.cpu().numpy()
            lo, hi = (a, b) if lo is None else (np.minimum(lo, a), np.maximum(hi, b))
    return lo, hi


def _fuse(method, dynamic, depth_all, ref_slot, src_slots, conf, img, mats, prob, num_consistent, dist_thresh, depth_thresh, stats):
    """one reference view for the mesh path: fusion.fuse_view, or with method="dynamic" fusion.fuse_view_dynamic.  Never with
    duplicate suppression: the volume averages every observation of a surface."""
    if fusion._check_method(method or "reference", dynamic, False):
        r = fusion.fuse_view(depth_all, ref_slot, src_slots, conf, img, mats, prob, num_consistent, dist_thresh, depth_thresh)
    else:
        r, _ = fusion._fuse_dyn(depth_all, ref_slot, src_slots, conf, img, mats, prob, method, dynamic, None, None)
    if stats is not None:
        stats["kept"] = stats.get("kept", 0) + int((r["masks"][2] != 0).sum())
    return r


def _fusion_argument(method, dynamic):
    """-> the keywords filtered_views takes for a fusion method that was asked for, and the dict its counts go to; nothing when none was"""
    if method is None and dynamic is None:
        return {}, None
    stats = {}
    return {"method": method or "reference", "dynamic": dynamic, "stats": stats}, stats


def _with_fusion(summary, method, dynamic, stats, fixed):
    if stats is not None:
        summary["fusion"] = fusion.fusion_summary({"method": method or "reference", "dynamic": dynamic, "dedup": False}, stats, fixed)
    return summary


def filtered_views(pair_folder, scan_folder, out_folder, prob_threshold, num_consistent, img_dist_thresh, depth_thresh, num_stage=3,
                   device="cuda:0", method="reference", dynamic=None, stats=None):
    """fusion.fuse_view per reference view of pair.txt, as filter_depth runs it -> dict: depth (V,H,W) fp32 = depth_avg where the
    final mask holds and 0 elsewhere, rgb (V,H,W,3) uint8, both on the device; cams (V,16) float64; lo, hi: the bounding box of
    the surviving points (float64, None when no point survives); ids: the V reference views' numbers in pair.txt's order.
    method / dynamic: filter_depth's; there is no dedup here, the volume wants every observation.  stats: a dict that receives the
    number of pixels kept as "kept" (one more host read per view)."""
    dev = torch.device(device)
    pairs = scan_io.read_pair_file(os.path.join(pair_folder, "pair.txt"))
    views = sorted({v for ref, srcs in pairs for v in [ref] + list(srcs)})
    slot = {v: i for i, v in enumerate(views)}
    cams = {v: scan_io.read_camera_parameters(os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v))) for v in views}
    depth_all = torch.from_numpy(np.stack([read_pfm(os.path.join(out_folder, "depth_est/{:0>8}.pfm".format(v)))[0] for v in views])).to(dev)
    depths, colours, rows, lo, hi = [], [], [], None, None
    for ref, srcs in pairs:
        if len(srcs) > fusion.MAX_SRC:
            raise _lib.RcmvsError(f"mesh_scan: view {ref} lists {len(srcs)} source views (at most {fusion.MAX_SRC})")
        conf = torch.from_numpy(read_pfm(os.path.join(out_folder, "confidence/{:0>8}.pfm".format(ref)))[0]).to(dev)
        img = scan_io.read_img(os.path.join(scan_folder, "images/{:0>8}.jpg".format(ref)))
        img = torch.from_numpy(fusion.stage_colour(img, num_stage, conf.shape)).to(dev)
        mats = torch.from_numpy(fusion.fusion_matrices(cams[ref][0], cams[ref][1], [cams[s][0] for s in srcs], [cams[s][1] for s in srcs])).to(dev)
        r = _fuse(method, dynamic, depth_all, slot[ref], [slot[s] for s in srcs], conf, img, mats, prob_threshold, num_consistent, img_dist_thresh,
                  depth_thresh, stats)
        lo, hi = _add_view(r, cams[ref], depths, colours, rows, lo, hi)
    return {"depth": torch.stack(depths).contiguous(), "rgb": torch.stack(colours).contiguous(), "cams": np.stack(rows), "lo": lo, "hi": hi,
            "ids": [int(ref) for ref, _ in pairs]}


def filtered_views_tanks(scan_folder, out_folder, geo_pixel_thres, geo_depth_thres, photo_thres, img_wh, image_sizes, geo_mask_thres,
                         device="cuda:0", depth_maps=None, conf_maps=None, method="reference", dynamic=None, stats=None):
    """filtered_views for a Tanks-and-Temples scene, as fusion.filter_depth_tanks runs the filter: cams_1/ with the intrinsics
    rescaled to ``img_wh``, the image resized by prepare_image, depth_maps / conf_maps optionally still on the device."""
    from PIL import Image
    from .mvs_dataset import prepare_image
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    pairs = scan_io.read_pair_file(os.path.join(scan_folder, "pair.txt"))
    views = sorted({v for ref, srcs in pairs for v in [ref] + list(srcs)})
    slot = {v: i for i, v in enumerate(views)}
    ow, oh = image_sizes
    cams = {}
    for v in views:
        K, E = scan_io.read_camera_parameters(os.path.join(scan_folder, "cams_1/{:0>8}_cam.txt".format(v)))
        K[0] *= img_wh[0] / ow
        K[1] *= img_wh[1] / oh
        cams[v] = (K, E)

    def plane(maps, v, kind):
        t = fusion._resident(maps, v, dev, kind)
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(read_pfm(os.path.join(out_folder, "{}/{:0>8}.pfm".format(kind, v)))[0])).to(dev)
        return t

    depth_all = torch.stack([plane(depth_maps, v, "depth_est") for v in views])
    if tuple(depth_all.shape[1:]) != (img_wh[1], img_wh[0]):
        raise _lib.RcmvsError(f"mesh_scan_tanks: depth maps are {tuple(depth_all.shape[1:])}, img_wh says {(img_wh[1], img_wh[0])}")
    depths, colours, rows, lo, hi = [], [], [], None, None
    for ref, srcs in pairs:
        if len(srcs) > fusion.MAX_SRC:
            raise _lib.RcmvsError(f"mesh_scan_tanks: view {ref} lists {len(srcs)} source views (at most {fusion.MAX_SRC})")
        conf = plane(conf_maps, ref, "confidence")
        raw = np.array(Image.open(os.path.join(scan_folder, "images/{:0>8}.jpg".format(ref))), dtype=np.uint8)
        img = prepare_image(raw, (img_wh[1], img_wh[0]), dev, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)).permute(1, 2, 0).contiguous()
        mats = torch.from_numpy(fusion.fusion_matrices(cams[ref][0], cams[ref][1], [cams[s][0] for s in srcs], [cams[s][1] for s in srcs])).to(dev)
        r = _fuse(method, dynamic, depth_all, slot[ref], [slot[s] for s in srcs], conf, img, mats, photo_thres, geo_mask_thres, geo_pixel_thres,
                  geo_depth_thres, stats)
        lo, hi = _add_view(r, cams[ref], depths, colours, rows, lo, hi)
    return {"depth": torch.stack(depths).contiguous(), "rgb": torch.stack(colours).contiguous(), "cams": np.stack(rows), "lo": lo, "hi": hi,
            "ids": [int(ref) for ref, _ in pairs]}


def mesh_scan_tanks(scan_folder, out_folder, meshfilename, geo_pixel_thres, geo_depth_thres, photo_thres, img_wh, image_sizes, geo_mask_thres,
                    n_views=None, scan="", device="cuda:0", depth_maps=None, conf_maps=None, voxel=None, resolution=1024, trunc_voxels=3.0,
                    min_weight=1, bounds=None, min_faces=0, min_fraction=0.0, keep_largest=0, smooth=0, decimate_cell=0.0, decimate_voxels=0.0, fill_holes=0,
                    render_dir=None, normals=None, texture=False, texture_size=None, simplify_faces=0, simplify_ratio=0.0, simplify_max_error=None,
                    method=None, dynamic=None):
    """The mesh counterpart of fusion.filter_depth_tanks, with its arguments: the scene's filtered ``depth_avg`` maps integrated into
    a SparseTsdfVolume (always sparse: these are the scenes a dense box does not fit) and meshed into ``meshfilename``.  Where no
    point survives the filter and no bounds are given there is nothing to put a grid round: the PLY is written empty, as
    filter_depth_tanks writes an empty cloud, and the summary says so.  method / dynamic: as mesh_scan's."""
    fuse_kw, fstats = _fusion_argument(method, dynamic)
    fixed = (geo_mask_thres, geo_pixel_thres, geo_depth_thres)
    views = filtered_views_tanks(scan_folder, out_folder, geo_pixel_thres, geo_depth_thres, photo_thres, img_wh, image_sizes, geo_mask_thres,
                                 device, depth_maps, conf_maps, **fuse_kw)
    if bounds is None and views["lo"] is None:
        os.makedirs(os.path.dirname(os.path.abspath(meshfilename)), exist_ok=True)
        with open(meshfilename, "wb") as f:
            f.write(mesh_ply_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
        return _with_fusion({"mesh": meshfilename, "views": int(views["depth"].shape[0]), "vertices": 0, "faces": 0, "active_blocks": 0, "allocated_voxels": 0,
                             "skipped_pixels": 0, "empty": "no point survives the filter"}, method, dynamic, fstats, fixed)
    return _with_fusion(_mesh_views(views, meshfilename, voxel, resolution, trunc_voxels, min_weight, bounds, True, device,
                       mesh_clean.clean_options(min_faces, min_fraction, keep_largest, smooth, fill_holes), **_decimate_argument(decimate_cell, decimate_voxels),
                       **_simplify_argument(simplify_faces, simplify_ratio, simplify_max_error),
                       **_render_argument(render_dir), **_normals_argument(normals), **_texture_argument(texture, texture_size)), method, dynamic, fstats, fixed)


def _decimate_argument(cell, voxels):
    """-> the keyword that hands mesh_decimate.decimate_options to _mesh_views; nothing at all when neither option is given"""
    options = mesh_decimate.decimate_options(cell, voxels)
    return {} if options is None else {"decimate": options}


def _simplify_argument(faces, ratio, max_error):
    """-> the keyword that hands mesh_simplify.simplify_options to _mesh_views; nothing at all when neither target is given"""
    if not faces and not ratio and max_error is None:
        return {}
    from . import mesh_simplify
    options = mesh_simplify.simplify_options(faces, ratio, max_error)
    return {} if options is None else {"simplify": options}


def _render_argument(render_dir):
    """-> the keyword that hands the folder of the rendered views to _mesh_views; nothing at all without one"""
    return {} if render_dir is None else {"render": str(render_dir)}


def _normals_argument(weight):
    """-> the keyword that hands mesh_normals.normals_options to _mesh_views; nothing at all when the option is not given"""
    from . import mesh_normals
    options = mesh_normals.normals_options(weight)
    return {} if options is None else {"normals": options}


def _texture_argument(enabled, max_size):
    """-> the keyword that hands mesh_texture.texture_options to _mesh_views; nothing at all when the option is not given"""
    if not enabled:
        return {}
    from . import mesh_texture
    return {"texture": mesh_texture.texture_options(True, max_size)}


def plan_grid(lo, hi, voxel=None, resolution=256, trunc_voxels=3.0, pad=True):
    """The grid of a box lo .. hi (float64): voxel defaults to the longest side / resolution, trunc = trunc_voxels * voxel, the
    box is padded by trunc on every side (pad=False: explicit bounds are taken as they are) -> (origin, voxel, dims, trunc)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise _lib.RcmvsError(f"mesh_scan: bad bounds {lo} .. {hi}")
    if voxel is None:
        voxel = float((hi - lo).max()) / int(resolution)
    voxel = float(voxel)
    if not (math.isfinite(voxel) and voxel > 0 and math.isfinite(trunc_voxels) and trunc_voxels > 0):
        raise _lib.RcmvsError(f"mesh_scan: voxel {voxel}, trunc_voxels {trunc_voxels} (finite, positive; a box without extent needs --voxel)")
    trunc = float(trunc_voxels) * voxel
    if pad:
        lo, hi = lo - trunc, hi + trunc
    dims = [max(1, int(math.ceil(float(s) / voxel))) for s in (hi - lo)]
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise _lib.RcmvsError(f"mesh_scan: {dims[0]} x {dims[1]} x {dims[2]} voxels of {voxel} (at most 2^28): use larger voxels or tighter bounds")
    return [float(v) for v in lo], voxel, dims, trunc


def plan_sparse_grid(lo, hi, voxel=None, resolution=1024, trunc_voxels=3.0, pad=True):
    """plan_grid for a SparseTsdfVolume: the sides are rounded up to whole blocks of 8 voxels and the limit is 2^27 blocks, not
    2^28 voxels -> (origin, voxel, bdims, trunc)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise _lib.RcmvsError(f"mesh_scan: bad bounds {lo} .. {hi}")
    if voxel is None:
        voxel = float((hi - lo).max()) / int(resolution)
    voxel = float(voxel)
    if not (math.isfinite(voxel) and voxel > 0 and math.isfinite(trunc_voxels) and trunc_voxels > 0):
        raise _lib.RcmvsError(f"mesh_scan: voxel {voxel}, trunc_voxels {trunc_voxels} (finite, positive; a box without extent needs --voxel)")
    trunc = float(trunc_voxels) * voxel
    if pad:
        lo, hi = lo - trunc, hi + trunc
    sides = [float(s) / voxel for s in (hi - lo)]
    if not all(s < 8.0 * SP_MAX_BLOCKS for s in sides):
        raise _lib.RcmvsError(f"mesh_scan: voxels of {voxel} in a box of {hi - lo} (at most 2^27 blocks): use larger voxels or tighter bounds")
    bdims = [max(1, (int(math.ceil(s)) + SP_BLOCK - 1) // SP_BLOCK) for s in sides]
    if bdims[0] * bdims[1] * bdims[2] > SP_MAX_BLOCKS:
        raise _lib.RcmvsError(f"mesh_scan: {bdims[0]} x {bdims[1]} x {bdims[2]} blocks of 8^3 voxels of {voxel} (at most 2^27): use larger voxels or "
                              "tighter bounds")
    return [float(v) for v in lo], voxel, bdims, trunc


def _mesh_views(views, meshfilename, voxel, resolution, trunc_voxels, min_weight, bounds, sparse, device, clean=None, decimate=None, render=None,
                normals=None, texture=None, simplify=None):
    """Plans the grid, integrates the filtered views, extracts, cleans the mesh when ``clean`` (the keyword arguments of
    mesh_clean.clean_mesh) is given, then decimates it when ``decimate`` (of mesh_decimate.decimate_options) is given, then collapses
    edges when ``simplify`` (of mesh_simplify.simplify_options) is given, and writes
    the PLY; with ``render`` (a folder) renders the written mesh into the views it was fused from (rc_mvsnet_amd.mesh_render) and
    compares it with their filtered depth maps; with ``normals`` (of mesh_normals.normals_options) computes the vertex normals of
    the final mesh, writes them into the PLY and hands them to the render; with ``texture`` (of mesh_texture.texture_options) textures
    the final mesh from the views' images and cameras, writes the texcoords into the PLY and the atlas next to it as <name>.png, and
    hands both to the render -> the summary dict"""
    plan = plan_sparse_grid if sparse else plan_grid
    if bounds is not None:
        b = [float(v) for v in bounds]
        if len(b) != 6:
            raise _lib.RcmvsError("mesh_scan: bounds are xmin ymin zmin xmax ymax zmax")
        origin, voxel, dims, trunc = plan(b[:3], b[3:], voxel, resolution, trunc_voxels, pad=False)
    else:
        if views["lo"] is None:
            raise _lib.RcmvsError("mesh_scan: no point survives the filter, so there is no bounding box; give bounds")
        origin, voxel, dims, trunc = plan(views["lo"], views["hi"], voxel, resolution, trunc_voxels)
    extra = {}
    if sparse:
        vol = SparseTsdfVolume(origin, voxel, dims, device)
        vol.mark(views["depth"], views["cams"], trunc)
        vol.build()
        extra = {"bdims": dims, "active_blocks": vol.n_active, "allocated_voxels": vol.voxels, "skipped_pixels": vol.skipped}
        dims = vol.dims
    else:
        vol = TsdfVolume(origin, voxel, dims, device)
    vol.integrate(views["depth"], views["cams"], views["rgb"], trunc=trunc)
    verts, faces, rgb = vol.extract(min_weight)
    if clean is not None:
        verts, faces, rgb, stats = mesh_clean.clean_mesh(verts, faces, rgb, **clean)
        extra["clean"] = stats
    if decimate is not None:
        verts, faces, rgb, stats = mesh_decimate.decimate_mesh_path(verts, faces, rgb, decimate, voxel)
        extra["decimate"] = stats
    if simplify is not None:
        from . import mesh_simplify
        verts, faces, rgb, extra["simplify"] = mesh_simplify.simplify(verts, faces, rgb, **simplify)
    os.makedirs(os.path.dirname(os.path.abspath(meshfilename)), exist_ok=True)
    vertex_normals = None
    if normals is not None:
        from . import mesh_normals
        vertex_normals, extra["normals"] = mesh_normals.vertex_normals(verts, faces, normals["weight"])
    ply_extra = {} if vertex_normals is None else {"normals": vertex_normals}            # the keywords of mesh_ply_bytes and of render_views: none without an option
    render_extra = dict(ply_extra)
    if texture is not None:
        from . import mesh_texture
        from .depth_vis import save_png
        tex = mesh_texture.texture(verts, faces, rgb, views["rgb"], views["cams"], **texture)
        stem = os.path.splitext(os.path.abspath(meshfilename))[0]
        save_png(stem + ".png", tex["atlas"])
        ply_extra.update(texcoords=tex["uv"], texture_file=os.path.basename(stem) + ".png")
        render_extra["texture"] = (tex["atlas"], tex["texel"])
        extra["texture"] = dict(mesh_texture.summary(tex), file=stem + ".png")
    with open(meshfilename, "wb") as f:
        f.write(mesh_ply_bytes(verts, faces, rgb, **ply_extra))
    if render is not None:
        from . import mesh_render
        extra["render"] = mesh_render.render_views(verts, faces, rgb, views, render, **render_extra)
    referenced = int(torch.unique(faces).numel())
    return dict({"mesh": meshfilename, "origin": origin, "dims": dims, "voxel": voxel, "trunc": trunc, "min_weight": int(min_weight),
                 "views": int(views["depth"].shape[0]), "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]),
                 "unreferenced_vertices": int(verts.shape[0]) - referenced, "observed_voxels": int((vol.wsum >= float(min_weight)).sum())}, **extra)


def mesh_scan(pair_folder, scan_folder, out_folder, meshfilename, prob_threshold, num_consistent, img_dist_thresh, depth_thresh, num_stage=3,
              voxel=None, resolution=256, trunc_voxels=3.0, min_weight=1, bounds=None, device="cuda:0", sparse=False, min_faces=0, min_fraction=0.0,
              keep_largest=0, smooth=0, decimate_cell=0.0, decimate_voxels=0.0, fill_holes=0, render_dir=None, normals=None, texture=False,
              texture_size=None, simplify_faces=0, simplify_ratio=0.0, simplify_max_error=None, method=None, dynamic=None):
    """Mesh one scan laid out as fusion.filter_depth reads it into ``meshfilename``.  method ("reference" or "dynamic") / dynamic: the
    consistency check of the filter, as fusion.filter_depth takes them; either given, the summary gains "fusion".  There is no dedup
    here: the volume averages every observation of a surface, and duplicate suppression would keep one and drop the rest.  bounds: (xmin, ymin, zmin, xmax, ymax, zmax),
    default the bounding box of the points that survive the filter, padded by the truncation distance.  sparse: a SparseTsdfVolume
    planned by plan_sparse_grid (resolution None: 1024); the summary then also reports bdims, active_blocks, allocated_voxels and
    skipped_pixels.  min_faces, min_fraction, keep_largest, smooth, fill_holes: any of them given, mesh_clean.clean_mesh runs on the
    extracted mesh and the summary gains its stats as "clean" (with fill_holes, "holes" among them).  decimate_cell (world units) or decimate_voxels (in voxels of the volume), not
    both: mesh_decimate.decimate runs after the clean-up and the summary gains its stats as "decimate".  simplify_faces (a face count) or
    simplify_ratio (a fraction of the valid faces), not both, with simplify_max_error: mesh_simplify.simplify runs after the clean-up and the
    clustering, before normals and texture, and the summary gains its stats as "simplify".  render_dir: the written mesh is
    rendered into the views it was fused from (mesh_render.render_views: depth_mesh/ and render/ under that folder) and compared with
    their filtered depth maps; the summary gains the summed table as "render".  normals ('area' or 'sphere'): mesh_normals.vertex_normals
    runs last, on the mesh that is written; the PLY's vertex records gain nx ny nz, the summary gains the stats as "normals", and a
    render gains the smooth shade and the normal image.  texture: mesh_texture.texture runs last, on the mesh that is written, from the
    views' images and cameras (texture_size: the atlas's largest side, default 8192); the PLY's faces gain texcoords, the atlas is written
    next to it as <name>.png, the summary gains "texture", and a render gains the textured views.  Returns the summary dict."""
    fuse_kw, fstats = _fusion_argument(method, dynamic)
    views = filtered_views(pair_folder, scan_folder, out_folder, prob_threshold, num_consistent, img_dist_thresh, depth_thresh, num_stage, device, **fuse_kw)
    if resolution is None:
        resolution = 1024 if sparse else 256
    return _with_fusion(_mesh_views(views, meshfilename, voxel, resolution, trunc_voxels, min_weight, bounds, bool(sparse), device,
                       mesh_clean.clean_options(min_faces, min_fraction, keep_largest, smooth, fill_holes), **_decimate_argument(decimate_cell, decimate_voxels),
                       **_simplify_argument(simplify_faces, simplify_ratio, simplify_max_error),
                       **_render_argument(render_dir), **_normals_argument(normals), **_texture_argument(texture, texture_size)),
                        method, dynamic, fstats, (num_consistent, img_dist_thresh, depth_thresh))


def main(argv=None):
    ap = argparse.ArgumentParser(description="TSDF fusion + marching tetrahedra of one scan's depth maps into a PLY mesh")
    ap.add_argument("--pair-folder", required=True, help="folder of pair.txt")
    ap.add_argument("--scan-folder", required=True, help="folder of cams/ and images/")
    ap.add_argument("--out-folder", required=True, help="folder of depth_est/ and confidence/")
    ap.add_argument("--mesh", required=True, help="the PLY to write")
    ap.add_argument("--prob_thres", type=float, default=0.8)
    ap.add_argument("--num_consistency", type=int, default=3)
    ap.add_argument("--img_dist_thres", type=float, default=0.5)
    ap.add_argument("--depth_thres", type=float, default=0.01)
    ap.add_argument("--num-stage", type=int, default=3)
    ap.add_argument("--voxel", type=float, default=None, help="voxel edge in world units (default: longest side / --resolution)")
    ap.add_argument("--resolution", type=int, default=None, help="default 256, with --sparse 1024")
    ap.add_argument("--sparse", action="store_true", help="a block-sparse volume: 8^3-voxel blocks allocated around the depth samples")
    ap.add_argument("--trunc-voxels", type=float, default=3.0, help="truncation distance in voxels")
    ap.add_argument("--min-weight", type=int, default=1, help="views a voxel must have been seen by")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("XMIN", "YMIN", "ZMIN", "XMAX", "YMAX", "ZMAX"))
    ap.add_argument("--min-faces", type=int, default=0, help="clean-up: drop components with fewer faces")
    ap.add_argument("--min-fraction", type=float, default=0.0, help="clean-up: drop components below this fraction of the largest one's faces")
    ap.add_argument("--keep-largest", type=int, default=0, help="clean-up: keep only the K components with most faces")
    ap.add_argument("--smooth", type=int, default=0, help="clean-up: rounds of Taubin smoothing")
    ap.add_argument("--fill-holes", type=int, default=0, help="clean-up: close boundary loops of at most N edges (rc_mvsnet_amd.mesh_holes; 0: none)")
    dec = ap.add_mutually_exclusive_group()
    dec.add_argument("--decimate-cell", type=float, default=0.0, help="decimation: edge of the clustering cells, world units")
    dec.add_argument("--decimate-voxels", type=float, default=0.0, help="decimation: edge of the clustering cells in voxels of the volume")
    sim = ap.add_mutually_exclusive_group()
    sim.add_argument("--simplify-faces", type=int, default=0, help="edge collapse (rc_mvsnet_amd.mesh_simplify) down to this many faces")
    sim.add_argument("--simplify-ratio", type=float, default=0.0, help="edge collapse down to this fraction of the faces")
    ap.add_argument("--simplify-max-error", type=float, default=None, help="edge collapse: no collapse above this cost (needs one of the two targets)")
    ap.add_argument("--render", default=None, metavar="DIR", help="render the written mesh into the views it was fused from (rc_mvsnet_amd.mesh_render): "
                                                                  "DIR/depth_mesh/*.pfm, DIR/render/*.png, and \"render\" in the summary")
    ap.add_argument("--normals", choices=("area", "sphere"), default=None, help="write oriented vertex normals (rc_mvsnet_amd.mesh_normals) into the PLY; "
                                                                                "with --render also <view>_smooth.png and <view>_normal.png")
    ap.add_argument("--texture", action="store_true", help="texture the written mesh from the views' images (rc_mvsnet_amd.mesh_texture): texcoords in the "
                                                           "PLY, the atlas next to it as <name>.png; with --render also <view>_tex.png")
    ap.add_argument("--texture-size", type=int, default=None, metavar="N", help="the atlas's largest side (default 8192, at most 16384)")
    ap.add_argument("--device", default="cuda:0")
    fusion.add_fusion_arguments(ap, dedup=False)
    ap.add_argument("--fusion-dedup", action="store_true", help="refused: the volume wants every observation (fuse the cloud with eval_driver --fusion-dedup)")
    a = ap.parse_args(argv)
    if a.fusion_dedup:
        raise SystemExit("tsdf_mesh: --fusion-dedup is for point clouds: the TSDF volume averages EVERY observation of a surface, and suppression "
                         "keeps one view's sample of it and drops the rest")
    fopt = fusion.fusion_options(a, "tsdf_mesh")
    summary = mesh_scan(a.pair_folder, a.scan_folder, a.out_folder, a.mesh, a.prob_thres, a.num_consistency, a.img_dist_thres, a.depth_thres,
                        num_stage=a.num_stage, voxel=a.voxel, resolution=a.resolution, trunc_voxels=a.trunc_voxels, min_weight=a.min_weight,
                        bounds=a.bounds, device=a.device, sparse=a.sparse, min_faces=a.min_faces, min_fraction=a.min_fraction,
                        keep_largest=a.keep_largest, smooth=a.smooth, decimate_cell=a.decimate_cell, decimate_voxels=a.decimate_voxels,
                        fill_holes=a.fill_holes, render_dir=a.render, normals=a.normals, **({"texture": True, "texture_size": a.texture_size} if a.texture else {}),
                        **({"simplify_faces": a.simplify_faces, "simplify_ratio": a.simplify_ratio, "simplify_max_error": a.simplify_max_error}
                           if (a.simplify_faces or a.simplify_ratio or a.simplify_max_error is not None) else {}),
                        **({"method": fopt["method"], "dynamic": fopt["dynamic"]} if fopt else {}))
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
