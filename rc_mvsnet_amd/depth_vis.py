"""The colour-mapped depth image of the reference's Tanks-and-Temples evaluation (``write_depth_img_2``,
eval_rcmvsnet_tanks.py:141-154) on the device: ``depth_colormap`` is that function up to ``Image.fromarray`` -- minimum, numpy's
95th percentile (exact: a radix select, csrc/depth_colormap.hip), ``Normalize``, ``magma_r``, truncation to 8 bits -- as four
launches on the current stream with no host read in between; ``write_depth_img_2`` adds the copy to the host and the PNG encoder
and is what the evaluation driver's writer threads run.  DESIGN.md section 4, "Tanks and Temples evaluation".

No CPU path: the map must be on the GPU.  No matplotlib import: the colour table is data of this package (``MAGMA_R``).
"""
import os

import numpy as np
import torch

from . import _lib
from .ops import _chk, _stream

# matplotlib's 'magma_r' (CC0), its 256 entries as trunc(rgb * 255): what ``(to_rgba(x)[:, :, :3] * 255).astype(uint8)`` can return.
# Generated once from matplotlib 3.10.8; tests/test_tanks_eval_cpu.py compares it with the installed matplotlib.
MAGMA_R = np.frombuffer(bytes.fromhex(
    "fbfcbffbfabdfbf9bbfbf7b9fcf5b7fcf3b5fcf1b3fcf0b1fceeb0fcecaefceaacfce8aafce6a8fce5a6fce3a5fde1a3"
    "fddfa1fddd9ffddc9dfdda9cfdd89afdd698fdd497fdd295fdd193fdcf92fdcd90fecb8efec98dfec78bfec689fec488"
    "fec286fec085febe83febc82febb80feb97ffeb77dfeb57cfeb37bfeb179feaf78feae76feac75feaa74fea873fea671"
    "fda470fda26ffda16efd9f6cfd9d6bfd9b6afd9969fd9768fd9567fc9366fc9265fc9064fc8e63fc8c63fb8a62fb8861"
    "fb8660fb8460fa825ffa805efa7f5ef97d5df97b5df9795cf8775cf8755cf7735cf7715bf6705bf66e5bf56c5bf56a5b"
    "f4685bf3675bf3655cf2635cf1615cf0605def5e5dee5d5dee5b5eed595fec585feb5660ea5560e85461e75262e65162"
    "e55063e44e64e24d65e14c66e04b66de4a67dd4968dc4869da4769d9466ad7456bd6446cd4436dd3426dd1426ed0416f"
    "ce4070cd3f70cb3e71ca3e72c83d72c63c73c53c74c33b74c23a75c03a75be3976bd3977bb3877b93778b83778b63679"
    "b53679b3357ab1357ab0347bae347bac337bab337ca9327ca7317da6317da4307da3307ea12f7e9f2f7e9e2e7e9c2e7f"
    "9a2d7f992d7f972c7f952c80942b80922b80912a808f2a808d29808c29808a2881892881872781852681842681822581"
    "8125817f24817e24817c23817a2281792281772181762181742081731f81711f816f1e816e1e816c1d806b1c80691c80"
    "681b80661a80651a8063197f61187f60187f5e177f5d177e5b167e5a157e58157e57147d55137d53137c52127c50127b"
    "4f117b4d117a4b10794a1079481078470f77450f76430f75420f74400f733e0f723c0f713b0f6f390f6e370f6c350f6a"
    "3410683210673010652f10622d10602b115e2a115c28115926115725115523115222115020114d1f114b1e10491c1046"
    "1b10441a1041180f3f170f3c160e3a150e38140d35120d33110c31100c2f0f0b2c0e0a2a0d0a280c09260b08240a0722"
    "09071f08061d07051b06051905041704041504031303031102020f02020d01010b010109010007000006000004000003"), dtype=np.uint8).reshape(256, 3)

_DEVICE = {}        # device -> (workspace, table): one per device, shared by every call on that device's current stream


def _device_state(device, lut):
    key = str(device)
    st = _DEVICE.get(key)
    if st is None:
        nbytes = _lib.load().rcmvs_depth_colormap_workspace_bytes()
        st = _DEVICE[key] = {"ws": torch.zeros(nbytes, dtype=torch.uint8, device=device), "luts": {}}
    lk = id(lut)
    if lk not in st["luts"]:
        table = np.ascontiguousarray(lut)
        if table.shape != (256, 3) or table.dtype != np.uint8:
            raise _lib.RcmvsError(f"depth_colormap: lut must be (256, 3) uint8, got {table.shape} {table.dtype}")
        if len(st["luts"]) >= 8:
            st["luts"].clear()
        st["luts"][lk] = (lut, torch.from_numpy(table.copy()).to(device))      # the key's object is kept alive with its copy
    return st["ws"], st["luts"][lk][1]


def reset():
    """Forget the cached workspaces and tables."""
    _DEVICE.clear()


def depth_colormap(depth, percentile=95.0, lut=MAGMA_R, return_stats=False):
    """depth (H,W) fp32 on the device -> rgb (H,W,3) uint8 on the device, (vmin, vmax) a device fp32 tensor of 2.
    No host synchronisation.  return_stats=True: the third value is the kernel's 4-float record (vmin, vmax, NaN flag, 0)."""
    if depth.dim() != 2 or depth.numel() == 0:
        raise _lib.RcmvsError(f"depth_colormap: depth must be (H, W) with H, W >= 1, got {tuple(depth.shape)}")
    if not 0.0 <= float(percentile) <= 100.0:
        raise _lib.RcmvsError(f"depth_colormap: percentile {percentile} is outside [0, 100]")
    H, W = depth.shape
    ws, table = _device_state(depth.device, lut)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=depth.device)
    stats = torch.empty(4, dtype=torch.float32, device=depth.device)
    _lib.call("rcmvs_depth_colormap", _chk(depth, "depth"), H, W, float(percentile), _chk(table, "lut", torch.uint8),
              _chk(rgb, "rgb", torch.uint8), _chk(stats, "stats"), _chk(ws, "workspace", torch.uint8),
              _stream())
    return (rgb, stats[:2], stats) if return_stats else (rgb, stats[:2])


def save_png(filename, rgb):
    """The writer job: copy the finished device image to the host (the only copy of the colour map) and encode it."""
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    Image.fromarray(rgb.cpu().numpy()).save(filename, format="PNG")


def write_depth_img_2(filename, depth):
    """The reference's name and signature; depth: a device tensor or a numpy array (uploaded to the current device)."""
    if not isinstance(depth, torch.Tensor):
        depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).cuda()
    save_png(filename, depth_colormap(depth)[0])
