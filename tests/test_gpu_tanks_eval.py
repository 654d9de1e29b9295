"""The Tanks-and-Temples workflow on the MI355X: csrc/depth_colormap.hip against the reference's images of tests/golden/tanks_eval.npz
(byte for byte, the 1056 x 1920 map by CRC-32), against the CPU emulation on ragged sizes, the device hand-over of
filter_depth_tanks against the file path, and the driver end to end on a synthetic two-scene tree."""
import glob
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN, REPO
from rc_mvsnet_amd import depth_vis, eval_driver, fusion, synthetic
from rc_mvsnet_amd.data_io import read_pfm

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(GOLDEN, "tanks_eval.npz"))
FUSION = np.load(os.path.join(GOLDEN, "fusion.npz"))
DEV = "cuda:0"


def colour(depth, **kw):
    rgb, vm = depth_vis.depth_colormap(torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(DEV), **kw)
    return rgb.cpu().numpy(), vm.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


@pytest.mark.parametrize("name", [str(c) for c in GOLD["cases"]])
def test_golden_cases_equal_the_reference_in_every_byte(name):
    depth, want, vm = GOLD["case:%s:depth" % name], GOLD["case:%s:image" % name], GOLD["case:%s:vminmax" % name]
    rgb, got = colour(depth)
    print(name, depth.shape, "vmin/vmax", got, "reference", vm, "differing bytes", int((rgb != want).sum()))
    if name == "nan":
        assert np.isnan(got).all() and np.isnan(vm).all()
    else:
        assert same_bits(got, vm)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, want)


def test_full_size_case_and_repeat():
    H, W, seed = (int(x) for x in GOLD["full:dims"])
    depth = synthetic.depth_vis_map(H, W, seed)
    assert zlib.crc32(depth.tobytes()) == int(GOLD["full:depth_crc"])
    rgb, vm = colour(depth)
    print("vmin/vmax", vm, "reference", GOLD["full:vminmax"], "differing sampled bytes", int((rgb[::16, ::16] != GOLD["full:image"]).sum()))
    assert same_bits(vm, GOLD["full:vminmax"])
    assert np.array_equal(rgb[::16, ::16], GOLD["full:image"])
    assert zlib.crc32(np.ascontiguousarray(rgb).tobytes()) == int(GOLD["full:crc"])
    again, vm2 = colour(depth)
    assert np.array_equal(rgb, again) and same_bits(vm, vm2)


def test_gpu_equals_the_emulation_on_ragged_sizes(tmp_path):
    """three seeded ragged maps: the emulation runs in a child process (its routing is process-wide), the GPU here"""
    sizes = [(61, 149, 5), (7, 1031, 6), (257, 3, 7)]
    script = tmp_path / "emu.py"
    script.write_text(
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ctypes, numpy as np, torch, conftest\n"
        "sys.path.insert(0, %r)\n"
        "import build as emu_build\n"
        "from rc_mvsnet_amd import _lib, depth_vis, synthetic\n"
        "lib = ctypes.CDLL(emu_build.build(sys.argv[2], only=('depth_colormap', 'geometry')))\n"       # this kernel and the error string only: seconds
        "for name in ('rcmvs_depth_colormap', 'rcmvs_depth_colormap_workspace_bytes', 'rcmvs_last_error_string'):\n"
        "    getattr(lib, name).argtypes, getattr(lib, name).restype = _lib.SIGNATURES[name], _lib._RESTYPES.get(name, ctypes.c_int)\n"
        "_lib._lib = lib\n"
        "depth_vis._chk = lambda t, name, dtype=torch.float32: ctypes.c_void_p(t.data_ptr())\n"
        "depth_vis._stream = lambda: ctypes.c_void_p(0)\n"
        "out = {}\n"
        "for h, w, seed in %r:\n"
        "    rgb, vm = depth_vis.depth_colormap(torch.from_numpy(synthetic.depth_vis_map(h, w, seed=seed)))\n"
        "    out['rgb%%d' %% seed], out['vm%%d' %% seed] = rgb.numpy(), vm.numpy()\n"
        "np.savez(sys.argv[1], **out)\n" % (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "emu"), sizes))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    subprocess.run([sys.executable, str(script), str(tmp_path / "emu.npz"), str(tmp_path / "emu_build")], env=env, check=True)
    emu = np.load(str(tmp_path / "emu.npz"))
    for h, w, seed in sizes:
        rgb, vm = colour(synthetic.depth_vis_map(h, w, seed=seed))
        assert np.array_equal(rgb, emu["rgb%d" % seed]) and same_bits(vm, emu["vm%d" % seed]), (h, w)


def test_unaligned_map_and_guard_bytes():
    """a map 4 bytes off a 16-byte line takes the scalar loads; nothing is written past a ragged image"""
    depth = synthetic.depth_vis_map(33, 47, seed=4)
    want, _ = colour(depth)
    buf = torch.zeros(33 * 47 + 1, device=DEV)
    buf[1:] = torch.from_numpy(depth).to(DEV).ravel()
    off = buf[1:].view(33, 47)
    assert off.data_ptr() % 16 != 0
    assert np.array_equal(depth_vis.depth_colormap(off)[0].cpu().numpy(), want)


def test_resident_maps_give_the_same_cloud_as_the_files(tmp_path):
    V, h, w, oh, ow, seed, n_src = [int(x) for x in FUSION["tanks:dims"]]
    pix, dth, photo, ncons = [float(x) for x in FUSION["tanks:thresholds"]]
    s = synthetic.tanks_fusion_scan(V=V, hw=(h, w), orig_hw=(oh, ow), seed=seed, n_src=n_src)
    scan_folder = str(tmp_path / "tt" / "intermediate" / "Horse")
    outs = [str(tmp_path / "files" / "Horse"), str(tmp_path / "resident" / "Horse")]
    synthetic.write_tanks_fusion_scan(s, scan_folder, outs[0])
    args = (pix, dth, photo, (w, h), (ow, oh), int(ncons), V, "Horse")
    a = fusion.filter_depth_tanks(scan_folder, outs[0], outs[0] + ".ply", *args, device=DEV, verbose=False)
    depth = {v: torch.from_numpy(s["depth"][v]).to(DEV) for v in range(V)}
    conf = {v: torch.from_numpy(s["conf"][v]).to(DEV) for v in range(V)}
    os.makedirs(outs[1])
    b = fusion.filter_depth_tanks(scan_folder, outs[1], outs[1] + ".ply", *args, device=DEV, verbose=False, depth_maps=depth, conf_maps=conf)
    assert len(a[0]) > 100 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert open(outs[0] + ".ply", "rb").read() == open(outs[1] + ".ply", "rb").read()
    for m in sorted(os.listdir(os.path.join(outs[0], "mask"))):
        assert open(os.path.join(outs[0], "mask", m), "rb").read() == open(os.path.join(outs[1], "mask", m), "rb").read()


def tree_bytes(root):
    return {os.path.relpath(p, root): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(root, "**", "*"), recursive=True)) if os.path.isfile(p)}


def test_driver_end_to_end_on_the_synthetic_tree(tmp_path):
    """7 views per item, two scenes of 7 views at 64 x 96: the reference's layout, every .pfm.png equal to depth_colormap of the
    .pfm beside it, the file read-back giving the same clouds, and a second run giving identical files"""
    data = str(tmp_path / "tt")
    synthetic.write_tanks_tree(data, scenes=("Family", "Horse"), V=7, hw=(64, 96), orig_hw=(75, 100), n_src=6)
    common = ["--dataset", "tanks", "--testpath", data, "--scenes", "Family,Horse", "--num_view", "7", "--max_w", "96", "--max_h", "64",
              "--ndepths", "16,8,8", "--io_threads", "2"]
    runs = []
    for k, extra in enumerate(([], [], ["--resident-gb", "0"])):
        out, ply = str(tmp_path / ("exp%d" % k)), str(tmp_path / ("ply%d" % k))
        eval_driver.main(common + ["--outdir", out, "--plydir", ply] + extra)
        runs.append((tree_bytes(out), tree_bytes(ply)))
    files, clouds = runs[0]
    assert sorted(clouds) == ["Family.ply", "Horse.ply"]
    assert len(files) == 2 * 7 * (3 + 3)
    for s in ("Family", "Horse"):
        for v in range(7):
            stem = os.path.join(str(tmp_path / "exp0"), s, "depth_est", "%08d.pfm" % v)
            depth = read_pfm(stem)[0]
            assert depth.shape == (64, 96) and os.path.exists(os.path.join(str(tmp_path / "exp0"), s, "confidence", "%08d.pfm" % v))
            assert np.array_equal(np.array(Image.open(stem + ".png")), colour(depth)[0])
    assert runs[1] == runs[0]                                          # two runs: identical files
    assert runs[2] == runs[0]                                          # the file read-back: the same clouds, masks and maps
