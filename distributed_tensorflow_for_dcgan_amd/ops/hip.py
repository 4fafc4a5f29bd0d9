"""Loader and thin tensor-level wrappers for the gfx950 kernel library (``_dcgan_hip``).

The extension is built in-tree by ``csrc/build.py`` (``__graft_entry__.build()``). On a
machine with a GPU the HIP path is mandatory: if the extension is missing or was built
for another architecture, :func:`ext` raises instead of silently falling back to PyTorch.

The wrappers below run ONE op through a throw-away ``Program`` on the current torch
stream; they exist for unit tests and for the autograd modules in ``ops.functional``.
The training engine records its whole step into persistent programs instead
(``engine.hip_engine``).
"""
from __future__ import annotations

import importlib
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from ..models.config import same_out, same_pads

_EXT = None

ACT = {None: 0, "none": 0, "relu": 1, "lrelu": 2, "tanh": 3}
# objective ids of gan_loss / gemv_head / gemv_head_bn (kernels.h GAN_BCE, GAN_LSGAN, GAN_HINGE)
GAN_LOSS_IDS = {"bce": 0, "lsgan": 1, "hinge": 2}


class HipUnavailable(RuntimeError):
    pass


def ext():
    """Import the compiled extension (torch must be imported first so that the HIP runtime
    shared by torch and the extension is the one already loaded)."""
    global _EXT
    if _EXT is None:
        try:
            _EXT = importlib.import_module("distributed_tensorflow_for_dcgan_amd._dcgan_hip")
        except ImportError as e:  # pragma: no cover - depends on build state
            raise HipUnavailable(
                "native HIP extension _dcgan_hip is not built; run `python csrc/build.py` "
                "(or __graft_entry__.build()). Original error: %s" % e) from e
    return _EXT


def available() -> bool:
    try:
        ext()
        return torch.cuda.is_available()
    except HipUnavailable:
        return False


def stream_ptr(stream: Optional[torch.cuda.Stream] = None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def run(prog, streams: Optional[Sequence] = None, begin: int = 0, end: int = -1) -> None:
    if streams is None:
        streams = [torch.cuda.current_stream()]
    prog.run([stream_ptr(s) if not isinstance(s, int) else s for s in streams], begin, end)


def _p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else int(t.data_ptr())


# --------------------------------------------------------------------------- tile policy
CU_COUNT = 256
IGEMM_CFGS = {0: (128, 128), 1: (128, 64), 2: (64, 128), 3: (64, 64), 4: (32, 64), 5: (64, 32),
              6: (32, 32), 7: (128, 16), 8: (64, 16), 9: (256, 64)}
IGEMM3_TILES = {0: (128, 128), 1: (256, 64), 2: (64, 256), 3: (128, 64), 4: (64, 128), 5: (64, 64),
                6: (256, 128), 7: (128, 256), 8: (512, 64), 9: (256, 256)}  # 6..9: 8-wave (512-thread) workgroups
IGEMM3_WAVES = {6: 8, 7: 8, 8: 8, 9: 8}
IGEMM3_WM = {0: 2, 1: 4, 2: 1, 3: 2, 4: 2, 5: 2, 6: 4, 7: 2, 8: 8, 9: 4}  # waves along M (igemm3.hip tiles)
# LDS stages of igemm3 cfg 200+10k+id; k = 4, 5 (cfg 240..259): the ping-pong K loop (8-wave tiles,
# conv / deconv modes with Kc % 64 == 0)
IGEMM3_STAGES = (3, 2, 4, 5, 3, 2)


# halo K loop (igemm3.hip PP == 2, cfg 300 + 10 k + id, NS = (3, 2)[k], 4-wave tiles 0 / 3 / 4 / 5):
# deconv phases with the input window of a phase tile staged once per 64-channel chunk
HALO_IDS = (0, 3, 4, 5)
HALO_PIXELS = 224  # window buffer capacity (igemm3.hip HALO_WPW x 4 waves x 8 pixels)


def is_halo(cfg: int) -> bool:
    return 300 <= cfg < 320 and cfg % 10 in HALO_IDS


def igemm3_ns(cfg: int) -> int:
    if cfg >= 300:
        return 3 if cfg < 310 else 2
    return IGEMM3_STAGES[(cfg - 200) // 10]


def halo_ok(cfg: int, mode: int, Bn: int, Hout: int, Wout: int, Kc: int, bkn: bool = False, splits: int = 1) -> bool:
    """Whether a halo cfg can run this GEMM (mirrors csrc/bindings.cpp igemm_ex): a deconv with
    k-contiguous weights, whole 64-channel chunks (split-K over chunks), every phase tile covering
    whole images or whole rows of one image with an input window of <= HALO_PIXELS pixels."""
    if not is_halo(cfg) or mode != 1 or bkn or Kc % 64 or splits > Kc // 64:
        return False
    bm = IGEMM3_TILES[cfg % 10][0]
    for py in (0, 1):
        for px in (0, 1):
            Hq, Wq = (Hout - py + 1) // 2, (Wout - px + 1) // 2
            hw = Hq * Wq
            if hw <= 0:
                continue
            whole, rows = bm % hw == 0, hw % bm == 0 and bm % Wq == 0
            nimg, R = (bm // hw, Hq) if whole else (1, bm // max(1, Wq))
            if not (whole or rows) or nimg * (R + 2) * (Wq + 2) > HALO_PIXELS:
                return False
    return True


def igemm3_pp_ok(cfg: int, mode: int, Kc: int) -> bool:
    """Whether igemm3 cfg can run this GEMM: the ping-pong configs (240..259) need an 8-wave tile
    and whole 64-channel k-tiles of a conv / deconv (no im2col plain mode); the halo configs
    (300..319) are checked with the full geometry by halo_ok."""
    if cfg >= 300:
        return is_halo(cfg) and mode == 1 and Kc % 64 == 0
    if cfg < 240:
        return True
    return cfg % 10 in IGEMM3_WAVES and mode != 2 and Kc % 64 == 0


def igemm3_lds(cfg: int) -> int:
    """Operand-ring bytes of igemm3 cfg (the launch adds room when the epilogue needs more)."""
    bm, bn = IGEMM3_TILES[cfg % 10]
    if cfg >= 300:
        return 2 * HALO_PIXELS * 128 + igemm3_ns(cfg) * bn * 128
    return igemm3_ns(cfg) * (bm + bn) * 128


# fp32 build (igemm_f32.hip): the only tile family of that element type, cfg 200..203
IGEMM_F32_TILES = {200: (64, 64), 201: (128, 64), 202: (64, 16), 203: (128, 128)}


def tile_of(cfg: int, dtype: int = 0) -> Tuple[int, int]:
    """(BM, BN) of an igemm cfg: 0..9 (+100 LDS-DMA) igemm.hip, 200..239 igemm3.hip; dtype 2
    (fp32): igemm_f32.hip; 240..259 igemm3's ping-pong K loop."""
    if dtype == 2:
        return IGEMM_F32_TILES[cfg]
    if cfg >= 200:
        return IGEMM3_TILES[cfg % 10]
    return IGEMM_CFGS[cfg % 100]


def pick_igemm_f32(M: int, N: int, phases: int = 1, rows_per_group: Optional[int] = None,
                   target_blocks: int = 2 * CU_COUNT) -> Optional[Tuple[int, int]]:
    """(cfg, 1) for the fp32 implicit GEMM: the largest tile that still gives ~target_blocks
    workgroups (narrow 64x16 tile for N <= 16, e.g. the RGB layers); no split-K."""
    order = [202] if N <= 16 else ([203, 201, 200] if N >= 128 else [201, 200])
    best = None
    for c in order:
        bm, bn = IGEMM_F32_TILES[c]
        if rows_per_group is not None and rows_per_group % bm:
            continue
        best = c
        if -(-M // bm) * -(-N // bn) * phases >= target_blocks:
            break
    return None if best is None else (best, 1)


def bnb_fits(cfg: int) -> bool:
    """True when the tile's LDS can hold the fused BN-backward statistics scratch (epilogue.h)."""
    bm, bn = tile_of(cfg)
    if cfg < 200:
        return (bm + 8 * bn) * 4 + bm * (bn + 8) * 2 + 16384 <= 2 * (bm + bn) * 128
    nt = 64 * IGEMM3_WAVES.get(cfg % 10, 4)
    wm = IGEMM3_WM[cfg % 10]
    # igemm3: the row-lane scratch may alias the C tile (the store pass has read it by then);
    # (halo tiles have more LDS than this ring estimate, as csrc/bindings.cpp assumes too)
    lds = max(igemm3_ns(cfg) * (bm + bn) * 128, (bm + 2 * wm * bn) * 4 + bm * (bn + 8) * 2)
    return (bm + 2 * wm * bn) * 4 + max(bm * (bn + 8) * 2, 64 * nt) <= lds


WGRAD_CFGS = {0: (128, 128), 1: (64, 128), 2: (128, 64), 3: (64, 64), 4: (32, 64), 5: (64, 32), 6: (32, 32)}


def pick_igemm_cfg(M: int, N: int, phases: int = 1, rows_per_group: Optional[int] = None,
                   target_blocks: int = 2 * CU_COUNT) -> int:
    """Largest tile that still gives >= target_blocks workgroups (fill 256 CUs twice);
    BM must divide rows_per_group when per-group BN statistics are produced."""
    if N <= 16:
        order = [7, 8]
    else:
        order = [0, 1, 2, 3, 4, 5, 6]
    best = None
    for c in order:
        bm, bn = IGEMM_CFGS[c]
        if rows_per_group is not None and rows_per_group % bm != 0:
            continue
        if bn > 16 and N < bn and bn > 32 and c not in (5, 6):
            # avoid tiles wider than N (wasted MFMA columns) unless nothing else fits
            continue
        blocks = -(-M // bm) * -(-N // bn) * phases
        if best is None:
            best = c
        if blocks >= target_blocks:
            return c
        best = c
    return best  # None when no tile divides rows_per_group (caller computes stats separately)


def pick_igemm3(M: int, N: int, Kc: int, taps: int, phases: int = 1, rows_per_group: Optional[int] = None,
                target_blocks: int = 2 * CU_COUNT) -> Optional[Tuple[int, int]]:
    """(cfg, splits) heuristic for igemm3: the largest 64x64-per-wave tile that fits N, then
    split-K until ~target_blocks workgroups (each split keeps >= 4 K tiles). Two LDS stages
    (21x): every layer of the in-situ tuned 128x128 step moved from 3 stages to 2
    (profiles/r3/tune_insitu_128_r3.txt), as most 64x64 entries had."""
    if N >= 128:
        order = [210, 211, 213, 215]
    elif N >= 64:
        order = [211, 213, 215]
    else:
        return None
    kt = taps * -(-Kc // 64)
    for c in order:
        bm, bn = IGEMM3_TILES[c % 10]
        if rows_per_group is not None and rows_per_group % bm != 0:
            continue
        tiles = -(-M // bm) * -(-N // bn) * phases
        sp = 1
        while tiles * sp < target_blocks and kt // (sp * 2) >= 4 and sp < 8:
            sp *= 2
        if tiles * sp >= target_blocks // 2 or c == order[-1]:
            return c, sp
    return None


_TUNED = None
TUNED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "igemm_tuned.json")


def tuned_table() -> dict:
    """Per-layer tile choices measured on MI355X by ``benchmarks/bench_kernels.py --write``
    (key ``mode,Bn,Hin,Win,Kc,Hout,Wout,N`` -> "cfg:splits" (or a bare cfg): cfg < 200 is
    igemm.hip (+100 = LDS-DMA staging), 200..239 igemm3.hip)."""
    global _TUNED
    if _TUNED is None:
        _TUNED = {}
        path = os.environ.get("DCGAN_TUNED_PATH", TUNED_PATH)  # A/B of tile tables
        if os.environ.get("DCGAN_NO_TUNED") != "1" and os.path.exists(path):
            import json
            with open(path) as f:
                for k, v in json.load(f).items():
                    c, _, sp = str(v).partition(":")
                    _TUNED[k] = (int(c), int(sp or 1))
    return _TUNED


class GemmShape(NamedTuple):
    """One conv-shaped GEMM as ``Program.igemm_ex`` takes it: mode 0 = stride-2 conv (25 taps), 1 =
    deconv (4 sub-pixel phases), 2 = plain GEMM; bkn: the weights are read as [tap][K][N]. A value
    (no buffers): it owns the row / phase arithmetic that the tile policy, the tuned table and the
    size of every fused-statistics buffer share with ``igemm_ex`` (mtiles * nphases)."""
    mode: int
    Bn: int
    Hin: int
    Win: int
    Kc: int
    Hout: int
    Wout: int
    N: int
    bkn: bool = False

    @classmethod
    def fwd(cls, L, Bn: int) -> "GemmShape":
        """The forward GEMM of layer L (a ConvSpec) at batch Bn: D's convs read [tap][K][N] weights."""
        conv = L.kind == "conv"
        return cls(0 if conv else 1, Bn, L.in_hw, L.in_hw, L.cin, L.out_hw, L.out_hw, L.cout, conv)

    @classmethod
    def dgrad(cls, L, Bn: int) -> "GemmShape":
        """The data-gradient GEMM of layer L: the deconv of a conv layer, the conv of a deconv layer."""
        conv = L.kind == "conv"
        return cls(1 if conv else 0, Bn, L.out_hw, L.out_hw, L.cout, L.in_hw, L.in_hw, L.cin, not conv)

    @property
    def phases(self) -> int:
        return 4 if self.mode == 1 else 1

    @property
    def M(self) -> int:
        """Rows per phase (a deconv's largest phase: odd sizes round up)."""
        if self.mode == 1:
            return self.Bn * (-(-self.Hout // 2)) * (-(-self.Wout // 2))
        return self.Bn * self.Hout * self.Wout

    @property
    def key(self) -> str:
        """Key of the tuned table."""
        return "%d,%d,%d,%d,%d,%d,%d,%d" % self[:8]

    def plan(self, rows_per_group: Optional[int] = None, dtype: int = 0) -> Optional[Tuple[int, int]]:
        """(cfg, splits) of ``igemm_cfg_for``, looked up in the module at every call (the in-situ
        tuner replaces it to see each lookup)."""
        return igemm_cfg_for(*self[:8], rows_per_group, self.bkn, dtype=dtype)

    def stat_rows(self, cfg: int, dtype: int = 0) -> int:
        """Partial-statistics rows a stats-emitting launch with tile cfg writes (M tiles x phases)."""
        return -(-self.M // tile_of(cfg, dtype)[0]) * self.phases


def igemm_cfg_for(mode: int, Bn: int, Hin: int, Win: int, Kc: int, Hout: int, Wout: int, N: int,
                  rows_per_group: Optional[int] = None, bkn: bool = False,
                  dtype: int = 0) -> Optional[Tuple[int, int]]:
    """(cfg, splits) for one implicit-GEMM launch: the tuned entry when present and legal
    (weight layout, BN-statistics grouping), else the heuristics. None when no tile can
    produce group-aligned statistics (caller computes them in a separate pass). dtype 2 =
    the fp32 build (its own tile family, no tuned table)."""
    shape = GemmShape(mode, Bn, Hin, Win, Kc, Hout, Wout, N, bkn)
    M, phases, taps = shape.M, shape.phases, {0: 25, 1: 9}.get(mode, 1)
    if dtype == 2:
        if mode == 1 and rows_per_group is not None:
            return None
        return pick_igemm_f32(M, N, phases, rows_per_group)
    ent = tuned_table().get(shape.key)
    if ent is not None:
        cfg, sp = ent
        ok = (cfg >= 200 and igemm3_pp_ok(cfg, mode, Kc)) or (not bkn and sp == 1 and cfg % 100 in IGEMM_CFGS)
        if cfg >= 300:
            ok = halo_ok(cfg, mode, Bn, Hout, Wout, Kc, bkn, sp)
        if ok and (rows_per_group is None or rows_per_group % tile_of(cfg)[0] == 0):
            return cfg, sp
    if N % 8 == 0 and N >= 64:
        r = pick_igemm3(M, N, Kc, taps, phases, rows_per_group)
        if r is not None:
            return r
    if bkn:
        return None
    c = pick_igemm_cfg(M, N, phases, rows_per_group)
    return None if c is None else (c, 1)


def pick_wgrad(Mc: int, Nc: int, K: int, taps: int, target_blocks: int = 4 * CU_COUNT,
               dtype: int = 0) -> Tuple[int, int]:
    """(cfg, splits) for a weight-gradient GEMM of Mc x Nc per tap over K pixels (dtype 2:
    the fp32 kernel, one 64x64 tile for every cfg)."""
    if dtype == 2:
        tiles = -(-Mc // 64) * -(-Nc // 64) * taps
        kt = -(-K // 64)
        return 3, max(1, min(-(-target_blocks // tiles), max(1, kt // (16 if taps == 1 else 4))))
    if Mc >= 128 and Nc >= 128:
        cfg = 0
    elif Mc < 128 and Nc >= 128:
        cfg = 1 if Mc > 32 else 4
    elif Mc >= 128 and Nc < 128:
        cfg = 2 if Nc > 32 else 5
    elif Mc > 32 and Nc > 32:
        cfg = 3
    elif Nc > 32:
        cfg = 4
    elif Mc > 32:
        cfg = 5
    else:
        cfg = 6
    bm, bn = WGRAD_CFGS[cfg]
    tiles = -(-Mc // bm) * -(-Nc // bn) * taps
    kt = -(-K // 64)
    # plain (im2col'd, 1-tap) layers reduce over up to 2^18 pixels into a tiny 80 x 64 matrix:
    # >= 16 k-tiles per split keeps the slab traffic (splits x Mc x Nc fp32) and the reduce short
    min_kt = 16 if taps == 1 else 4
    splits = max(1, min(-(-target_blocks // tiles), max(1, kt // min_kt)))
    return cfg, splits


WGRAD3_TILES = {0: (128, 128), 1: (64, 128), 2: (128, 64), 3: (64, 64)}
# wgrad5.hip (csrc/hip/wgrad5.hip, cfg 400 + id): (Mc, BN, Wd, LDS stages) -- a workgroup owns one
# kernel row (5 taps) x all Mc x BN channels, a k-tile is 64 / Wd whole output rows of one image
WGRAD5_CFGS = {400: (64, 64, 16, 2), 401: (64, 64, 16, 3), 402: (64, 64, 8, 2), 403: (64, 64, 32, 2),
               404: (128, 64, 8, 2), 405: (128, 64, 16, 2), 406: (128, 32, 8, 2), 407: (128, 32, 16, 2),
               408: (64, 64, 64, 2), 409: (64, 64, 4, 2)}
# 410 + id: the same tiles with the split-K sum in a second, GPU-wide kernel (no last-arrival tail)
WGRAD5_CFGS.update({c + 10: v for c, v in list(WGRAD5_CFGS.items())})


def wgrad5_fits(cfg: int, Mc: int, Hd: int, Wd: int, Bn: int = 64) -> bool:
    """wgrad5 cfg usable for a layer: whole channel blocks, its output width, whole output rows
    per 64-pixel k-tile (a fraction of one image or whole images), whole k-tiles."""
    ent = WGRAD5_CFGS.get(cfg)
    if ent is None or Mc % ent[0] or ent[2] != Wd:
        return False
    R = 64 // Wd
    return (Hd % R == 0 or R % Hd == 0) and (Bn * Hd * Wd) % 64 == 0


def pick_wgrad3(Mc: int, Nc: int, K: int, target_blocks: int = 2 * CU_COUNT) -> Optional[Tuple[int, int]]:
    """(cfg, splits) heuristic for wgrad3.hip (25-tap gather GEMM, in-kernel split-K): the
    largest tile not wider than the operands, split-K until ~target_blocks workgroups while
    every split keeps >= 8 k-tiles of 64 pixels. None -> wgrad.hip."""
    if Mc % 8 or Nc % 8 or Mc < 64 or Nc < 64:
        return None
    kt = -(-K // 64)
    for tid in (0, 1, 2, 3):
        bm, bn = WGRAD3_TILES[tid]
        if bm > Mc or bn > Nc:
            continue
        tiles = -(-Mc // bm) * -(-Nc // bn) * 25
        sp = 1
        while tiles * sp < target_blocks and kt // (2 * sp) >= 8 and sp < 16:
            sp *= 2
        return 310 + tid, sp  # two LDS stages (31x), as every tuned 64x64 entry
    return None


def wgrad3_key(Mc: int, Nc: int, Bn: int, Hd: int, Wd: int, Hg: int) -> str:
    return "w3,%d,%d,%d,%d,%d,%d" % (Mc, Nc, Bn, Hd, Wd, Hg)


def wgrad_splits_for(Mc: int, Nc: int, Bn: int, Hd: int, Wd: int, Hg: int) -> Optional[int]:
    """Tuned split count for wgrad.hip on a 25-tap layer (entry "0:splits"), or None."""
    ent = tuned_table().get(wgrad3_key(Mc, Nc, Bn, Hd, Wd, Hg))
    return ent[1] if ent is not None and ent[0] == 0 and ent[1] >= 1 else None


def wgrad3_cfg_for(Mc: int, Nc: int, Bn: int, Hd: int, Wd: int, Hg: int) -> Optional[Tuple[int, int]]:
    """(cfg, splits) for a 25-tap weight gradient on wgrad3.hip, or None to keep wgrad.hip:
    the tuned entry (benchmarks/bench_wgrad.py --write; cfg 0 = wgrad.hip measured faster),
    else the heuristic."""
    if os.environ.get("DCGAN_NO_WGRAD3") == "1":
        return None
    ent = tuned_table().get(wgrad3_key(Mc, Nc, Bn, Hd, Wd, Hg))
    if ent is not None:
        return None if ent[0] == 0 else ent
    return pick_wgrad3(Mc, Nc, Bn * Hd * Wd)


# --------------------------------------------------------------------------- one-shot wrappers
def _check_bf16(*ts):
    for t in ts:
        if t is not None and (t.dtype not in (torch.bfloat16, torch.float16) or not t.is_contiguous()
                              or not t.is_cuda):
            raise ValueError("expected contiguous cuda bf16 tensor, got %s %s" % (t.dtype, t.device))


def pack_conv_weight(w: torch.Tensor, kind: str, use: str) -> torch.Tensor:
    """bf16 B-operand layout [25][N][Kc] for the igemm kernel.

    conv weight HWIO [5,5,ci,co]: use='fwd' -> [25][co][ci] (transposed), 'dgrad' -> natural.
    deconv weight [5,5,co,ci]:    use='fwd' -> natural,              'dgrad' -> [25][ci][co]."""
    w = w.reshape(25, w.shape[2], w.shape[3])
    transpose = (kind == "conv" and use == "fwd") or (kind == "deconv" and use == "dgrad")
    if transpose:
        w = w.transpose(1, 2)
    return w.contiguous().to(torch.bfloat16)


def pack_im2col_weight(w: torch.Tensor, kind: str, kpad: int) -> torch.Tensor:
    """[N][kpad] bf16 for a 3-channel layer run as a plain GEMM over im2col rows.
    conv (D L0) HWIO [5,5,3,co] -> Bt[co][tap*3+ci]; deconv dgrad (G last) [5,5,3,ci]:
    Bt[ci][tap*3+co]."""
    A = w.shape[2]
    t = w.reshape(25 * A, w.shape[3]).t()  # [N][25*A], k = tap*A + a
    out = torch.zeros(t.shape[0], kpad, dtype=torch.bfloat16, device=w.device)
    out[:, :25 * A] = t.to(torch.bfloat16)
    return out


def conv2d_same(x: torch.Tensor, w_packed: torch.Tensor, cout: int, bias: Optional[torch.Tensor] = None,
                act: Optional[str] = None, leak: float = 0.2, stats: bool = False, out_f32: bool = False,
                cfg: Optional[int] = None, bkn: bool = False, splits: int = 1):
    """TF-SAME stride-2 5x5 conv on the HIP igemm kernel. x bf16 NHWC [B,H,W,Ci] (Ci % 8 == 0),
    w_packed bf16 [25][co][ci] (bkn=True: [25][ci][co], i.e. the HWIO weight itself; cfg >= 200).
    Returns y (and per-tile stats partials [P,2,co] if stats)."""
    _check_bf16(x, w_packed)
    B, H, W, Ci = x.shape
    Ho, Wo = same_out(H), same_out(W)
    py, px = same_pads(H)[0], same_pads(W)[0]
    M = B * Ho * Wo
    cfg = pick_igemm_cfg(M, cout) if cfg is None else cfg
    bm, bn = tile_of(cfg)
    y = torch.empty(B, Ho, Wo, cout, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    mt = -(-M // bm)
    st = torch.empty(mt, 2, cout, device=x.device, dtype=torch.float32) if stats else None
    prog = ext().Program()
    prog.igemm_ex("conv", 0, _p(x), _p(w_packed), _p(y), B, H, W, Ci, Ho, Wo, cout, py, px, cfg, int(out_f32), cout,
                  0, _p(bias), ACT[act], leak, _p(st), 0, int(bkn), -1, splits)
    run(prog)
    return (y, st) if stats else y


def conv2d_transpose_same(x: torch.Tensor, w_packed: torch.Tensor, cout: int, out_hw: Tuple[int, int],
                          bias: Optional[torch.Tensor] = None, act: Optional[str] = None, leak: float = 0.2,
                          stats: bool = False, out_f32: bool = False, cfg: Optional[int] = None,
                          bkn: bool = False, splits: int = 1):
    """TF-SAME stride-2 5x5 conv_transpose via 4 sub-pixel phases. x bf16 [B,Hi,Wi,Ci],
    w_packed bf16 [25][co][ci] (bkn=True: [25][ci][co]; cfg >= 200)."""
    _check_bf16(x, w_packed)
    B, Hi, Wi, Ci = x.shape
    Ho, Wo = out_hw
    py, px = same_pads(Ho)[0], same_pads(Wo)[0]
    Mphase = B * (-(-Ho // 2)) * (-(-Wo // 2))
    cfg = pick_igemm_cfg(Mphase, cout, phases=4) if cfg is None else cfg
    bm, bn = tile_of(cfg)
    y = torch.empty(B, Ho, Wo, cout, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    prog = ext().Program()
    st = None
    if stats:
        mt = -(-Mphase // bm)
        st = torch.empty(mt * 4, 2, cout, device=x.device, dtype=torch.float32)
    prog.igemm_ex("deconv", 1, _p(x), _p(w_packed), _p(y), B, Hi, Wi, Ci, Ho, Wo, cout, py, px, cfg, int(out_f32),
                  cout, 0, _p(bias), ACT[act], leak, _p(st), 0, int(bkn), -1, splits)
    run(prog)
    return (y, st) if stats else y


NCONV_MAX_GRID = 512  # persistent workgroups of nconv (2 per CU: the kernel's occupancy)


def nconv_grid(prog, B: int, Ho: int, Wo: int, cap: Optional[int] = None) -> int:
    """Workgroup count of an nconv launch (= its BN-backward partial rows): persistent (cap
    workgroups looping over the tiles) or, with cap <= 0, one workgroup per tile. The default cap
    is NCONV_MAX_GRID; DCGAN_NCONV_CAP overrides it (A/B studies)."""
    if cap is None:
        v = os.environ.get("DCGAN_NCONV_CAP", str(NCONV_MAX_GRID))
        if not v.isdigit():
            raise ValueError("DCGAN_NCONV_CAP must be a non-negative integer (0 = one workgroup per tile), "
                             "got %r" % v)
        cap = int(v)
    tiles = prog.nconv_tiles(B, Ho, Wo)
    return tiles if cap <= 0 else min(tiles, cap)


def nconv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
          leak: float = 0.2, bnb: Optional[tuple] = None):
    """TF-SAME stride-2 5x5 conv with Cin <= 4 and Cout = 64 on narrow2.hip's persistent MFMA
    kernel. x [B,H,W,Cin], w HWIO [5,5,Cin,64]. bnb = (bx, by, mean[64], rstd[64], act): also
    the BN-backward partial statistics (sum g, sum g*xhat), g = y_out * act'(by) -- returned as
    [grid][2][64] next to the output."""
    _check_bf16(x, w)
    B, Hh, Ww, C = x.shape
    Ho, Wo = -(-Hh // 2), -(-Ww // 2)
    y = torch.empty(B, Ho, Wo, 64, device=x.device, dtype=x.dtype)
    prog = ext().Program(x.dtype == torch.float16)
    grid = nconv_grid(prog, B, Ho, Wo)
    part = torch.empty(grid, 2, 64, device=x.device) if bnb is not None else None
    bx, by, mean, rstd, bact = bnb if bnb is not None else (None, None, None, None, None)
    prog.nconv("nconv", _p(x), _p(w), _p(bias), _p(y), B, Hh, Ww, C, Ho, Wo, same_pads(Hh)[0], same_pads(Ww)[0],
               ACT[act], leak, grid, _p(bx), _p(by), _p(mean), _p(rstd), ACT[bact], leak, _p(part), 0)
    run(prog)
    return (y, part) if bnb is not None else y


def nwgrad(x: torch.Tensor, d: torch.Tensor, pad: int) -> torch.Tensor:
    """Weight gradient of a 1..4-channel stride-2 5x5 layer (narrow2.hip): out[25][Cin][64] =
    sum over d's pixels of the stride-2 window of x (top/left padding `pad`) times d."""
    _check_bf16(x, d)
    B, Hh, Ww, C = x.shape
    _, Hd, Wd, N = d.shape
    assert N == 64
    out = torch.empty(25, C, 64, device=x.device)
    prog = ext().Program(x.dtype == torch.float16)
    prog.nwgrad("nwgrad", _p(x), B, Hh, Ww, C, _p(d), Hd, Wd, pad, _p(out), 0)
    run(prog)
    return out


def narrow_deconv(x: torch.Tensor, w: torch.Tensor, out_hw: Tuple[int, int], bias: Optional[torch.Tensor] = None,
                  act: Optional[str] = None, leak: float = 0.2) -> torch.Tensor:
    """TF-SAME stride-2 5x5 conv_transpose with N <= 4 output channels on the direct VALU
    kernel. x [B,Hi,Wi,C] (C % 8 == 0), w [25][N][C] (the TF deconv layout [5,5,N,C], or a
    conv's HWIO [5,5,N=ci,C=co] for its data gradient)."""
    _check_bf16(x, w)
    B, Hi, Wi, C = x.shape
    N = w.numel() // (25 * C)
    Ho, Wo = out_hw
    y = torch.empty(B, Ho, Wo, N, device=x.device, dtype=x.dtype)
    prog = ext().Program(x.dtype == torch.float16)
    prog.narrow_deconv("narrow", _p(x), _p(w), _p(bias), _p(y), B, Hi, Wi, C, Ho, Wo, N, same_pads(Ho)[0],
                       ACT[act], leak, 0)
    run(prog)
    return y


def gemm_plain(a: torch.Tensor, bt: torch.Tensor, out_f32: bool = False, bias=None, act=None,
               cfg: Optional[int] = None, bkn: bool = False, splits: int = 1) -> torch.Tensor:
    """C[M][N] = A[M][K] . Bt[N][K] (bf16, K % 8 == 0). bkn=True: bt is B[Kb][N] (n contiguous,
    Kb <= K rows; rows Kb..K-1 read as zeros -- the im2col K padding)."""
    _check_bf16(a, bt)
    M, K = a.shape
    N = bt.shape[1] if bkn else bt.shape[0]
    kb = bt.shape[0] if bkn else -1
    cfg = pick_igemm_cfg(M, N) if cfg is None else cfg
    c = torch.empty(M, N, device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    prog = ext().Program()
    prog.igemm_ex("gemm", 2, _p(a), _p(bt), _p(c), M, 1, 1, K, 1, 1, N, 0, 0, cfg, int(out_f32), N, 0, _p(bias),
                  ACT[act], 0.2, 0, 0, int(bkn), kb, splits)
    run(prog)
    return c


def conv_wgrad(g_src: torch.Tensor, dm: torch.Tensor, pad: int, mode: int = 0, cfg=None, splits=None) -> torch.Tensor:
    """out[25][Mc][Nc] = sum_k G[b,2y+ky-pad,2x+kx-pad,m] * Dm[b,y,x,n] (fp32).
    mode 2: g_src is an im2col matrix [K][Mc] and the result is [Mc][Nc]."""
    _check_bf16(g_src, dm)
    if mode == 2:
        K, Mc = g_src.shape
        Nc = dm.shape[-1]
        Bn, Hd, Wd = K, 1, 1
        Hg = Wg = 1
        taps = 1
    else:
        Bn, Hg, Wg, Mc = g_src.shape
        _, Hd, Wd, Nc = dm.shape
        taps = 25
        K = Bn * Hd * Wd
    c, s = pick_wgrad(Mc, Nc, K, taps)
    cfg = c if cfg is None else cfg
    splits = s if splits is None else splits
    slabs = torch.empty(splits, taps, Mc, Nc, device=dm.device, dtype=torch.float32)
    out = torch.empty(taps, Mc, Nc, device=dm.device, dtype=torch.float32)
    prog = ext().Program()
    prog.wgrad("wgrad", mode, _p(g_src), Hg, Wg, Mc, _p(dm), Bn, Hd, Wd, Nc, pad, cfg, splits, _p(slabs), _p(out),
               out.numel(), 1.0, 0)
    run(prog)
    return out if mode != 2 else out[0]


def conv_wgrad3(g_src: torch.Tensor, dm: torch.Tensor, pad: int, cfg: Optional[int] = None,
                splits: Optional[int] = None, scale: float = 1.0) -> torch.Tensor:
    """wgrad3.hip: out[25][Mc][Nc] = scale * sum_k G[b,2y+ky-pad,2x+kx-pad,m] * Dm[b,y,x,n] (fp32)."""
    _check_bf16(g_src, dm)
    Bn, Hg, Wg, Mc = g_src.shape
    _, Hd, Wd, Nc = dm.shape
    if cfg is None or splits is None:
        plan = pick_wgrad3(Mc, Nc, Bn * Hd * Wd)
        if plan is None:
            raise ValueError("no wgrad3 tile for Mc=%d Nc=%d" % (Mc, Nc))
        cfg = plan[0] if cfg is None else cfg
        splits = plan[1] if splits is None else splits
    out = torch.empty(25, Mc, Nc, device=dm.device, dtype=torch.float32)
    prog = ext().Program(g_src.dtype == torch.float16)
    prog.wgrad3("wgrad3", _p(g_src), Hg, Wg, Mc, _p(dm), Bn, Hd, Wd, Nc, pad, cfg, splits, _p(out), scale, 0)
    run(prog)
    return out


def act_bwd_dbias(dy: torch.Tensor, y: torch.Tensor, act: int, leak: float = 0.2):
    """(dx, db): dx = dy * act'(y) (elem dtype), db[c] = sum over rows of dx (fp32) -- one launch."""
    _check_bf16(dy, y)
    C = dy.shape[-1]
    R = dy.numel() // C
    dx = torch.empty_like(dy)
    db = torch.empty(C, device=dy.device, dtype=torch.float32)
    prog = ext().Program(dy.dtype == torch.float16)
    prog.act_bwd_dbias("abd", _p(dy), _p(y), _p(dx), R, C, act, leak, _p(db), 0)
    run(prog)
    return dx, db


def head_bwd(x: torch.Tensor, dl: torch.Tensor, w: torch.Tensor):
    """(dx, dW, db) of logits = x @ w + b: dW = x^T dl, db = sum dl, dx = dl w^T (elem dtype)."""
    _check_bf16(x)
    R, K = x.shape
    dx = torch.empty_like(x)
    dW = torch.empty(K, device=x.device, dtype=torch.float32)
    db = torch.empty(1, device=x.device, dtype=torch.float32)
    prog = ext().Program(x.dtype == torch.float16)
    prog.head_bwd("hb", _p(x), _p(dl), _p(w), _p(dx), _p(dW), _p(db), R, K, 0)
    run(prog)
    return dx, dW, db


def im2col_s2(x: torch.Tensor, kpad: int) -> torch.Tensor:
    _check_bf16(x)
    B, H, W, C = x.shape
    Ho, Wo = same_out(H), same_out(W)
    out = torch.empty(B * Ho * Wo, kpad, device=x.device, dtype=torch.bfloat16)
    prog = ext().Program()
    prog.im2col_s2("im2col", _p(x), _p(out), B, H, W, C, Ho, Wo, same_pads(H)[0], same_pads(W)[0], kpad, 0)
    run(prog)
    return out


def _lr_kw(sched, step: Optional[torch.Tensor], op: str, with_step: bool = True) -> dict:
    """Keyword arguments of an Adam op for a learning-rate schedule (ops.reference.LrSchedule)
    evaluated on the device from `step` (int64[1], the global step); {} when there is none."""
    if sched is None:
        return {}
    kw = dict(zip(("lr_kind", "lr_start", "lr_steps", "lr_end", "lr_warmup"), sched.hip_args()))
    if step is not None:
        if step.dtype != torch.int64 or step.numel() != 1:
            raise TypeError("%s: step must be one int64" % op)
        if with_step:
            kw["lr_step"] = _p(step)
    return kw


def lr_factor(steps: torch.Tensor, sched) -> torch.Tensor:
    """The schedule's factor at each step value, int64[N] -> float32[N], from the device function
    the Adam kernels evaluate (dcg::lr_factor)."""
    if steps.dtype != torch.int64:
        raise TypeError("lr_factor: steps must be int64")
    steps = steps.contiguous()
    out = torch.empty(steps.shape, device=steps.device, dtype=torch.float32)
    if steps.numel():
        prog = ext().Program()
        prog.lr_factor("lr_factor", _p(steps), _p(out), steps.numel(), *sched.hip_args())
        run(prog)
    return out


_ELEM_DT = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def _check_step(op: str, step: torch.Tensor) -> None:
    if step.dtype != torch.int64 or step.numel() != 1:
        raise TypeError("%s: step must be one int64" % op)


def philox_normal(n: int, seed: int, step: torch.Tensor, stream_id: int = 1) -> torch.Tensor:
    """float32[n] standard normals of the Philox stream (seed, step[0], stream_id), as the instance-noise
    kernel draws them (Box-Muller per pair of lanes; oracle: ops.reference.philox_normal)."""
    _check_step("philox_normal", step)
    out = torch.empty(int(n), device=step.device, dtype=torch.float32)
    if n:
        prog = ext().Program()
        prog.philox_normal("philox_normal", _p(out), int(n), int(seed), _p(step), int(stream_id))
        run(prog)
    return out


def noise_sigma(steps: torch.Tensor, sigma0: float, sigma1: float, nsteps: int) -> torch.Tensor:
    """sigma(t) of the instance-noise anneal at each step value, int64[N] -> float32[N], from the device
    function the noise kernel evaluates (dcg::noise_sigma)."""
    if steps.dtype != torch.int64:
        raise TypeError("noise_sigma: steps must be int64")
    steps = steps.contiguous()
    out = torch.empty(steps.shape, device=steps.device, dtype=torch.float32)
    prog = ext().Program()
    prog.noise_sigma("noise_sigma", _p(steps) if steps.numel() else 0, _p(out), steps.numel(), float(sigma0),
                     float(sigma1), int(nsteps))
    run(prog)
    return out


def instance_noise(x: torch.Tensor, y: torch.Tensor, seed: int, step: torch.Tensor, sigma0: float, sigma1: float,
                   nsteps: int, stream_id: int = 1) -> torch.Tensor:
    """y = x + sigma(step[0]) * eps elementwise over the flat buffer (bf16, fp16 or fp32; y a buffer of
    its own, same shape and dtype), eps the normals of the Philox stream (seed, step[0], stream_id)."""
    if x.dtype not in _ELEM_DT or y.dtype != x.dtype or y.shape != x.shape:
        raise TypeError("instance_noise: x and y must share a shape and a dtype of bf16, fp16 or fp32")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("instance_noise: x and y must be contiguous")
    _check_step("instance_noise", step)
    prog = ext().Program(_ELEM_DT[x.dtype])
    prog.instance_noise("instance_noise", _p(x) if x.numel() else 0, _p(y) if y.numel() else 0, x.numel(), int(seed),
                        _p(step), int(stream_id), float(sigma0), float(sigma1), int(nsteps))
    run(prog)
    return y


def _aug_images(op: str, x: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if x.dtype not in _ELEM_DT or x.dim() != 4 or x.shape[1] != x.shape[2]:
        raise TypeError("%s: x must be [N, S, S, C] in bf16, fp16 or fp32" % op)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    if out.dtype != x.dtype or out.shape != x.shape:
        raise TypeError("%s: out must have x's shape and dtype" % op)
    if not (x.is_contiguous() and out.is_contiguous()):
        raise ValueError("%s: x and out must be contiguous" % op)
    return out


def _ada_state_arg(op: str, p24, device) -> torch.Tensor:
    """The int32 [8] device state a gated launch reads p24 from: a given one, or a fresh one holding p24."""
    if torch.is_tensor(p24):
        if p24.dtype != torch.int32 or p24.numel() != 8 or not p24.is_contiguous() or p24.device != device:
            raise TypeError("%s: the state must be a contiguous int32 [8] on x's device" % op)
        return p24
    if not 0 <= int(p24) <= 1 << 24:
        raise ValueError("%s: p24 must satisfy 0 <= p24 <= 2^24, got %r" % (op, p24))
    return torch.tensor([int(p24)] + [0] * 7, dtype=torch.int32, device=device)


def _gates_arg(op: str, gates, N: int, device) -> torch.Tensor:
    if not torch.is_tensor(gates) or gates.numel() != N or gates.is_floating_point():
        raise TypeError("%s: gates must be an integer [N]" % op)
    return gates.to(device=device, dtype=torch.int32).contiguous()


def _int_rows(op: str, params: torch.Tensor, params_out, N: int, device) -> torch.Tensor:
    if tuple(params.shape) != (N, 4) or params.dtype not in (torch.int32, torch.int64):
        raise TypeError("%s: params must be an integer [N, 4]" % op)
    return params.to(device=device, dtype=torch.int32).contiguous()


def _color_rows(op: str, params: torch.Tensor, params_out, N: int, device) -> torch.Tensor:
    if params.dim() != 2 or params.shape[0] != N or params.shape[1] not in (3, 4) or not params.is_floating_point():
        raise TypeError("%s: params must be a floating-point [N, 3] or [N, 4]" % op)
    p = params_out
    if p is None:
        p = torch.zeros(N, 4, device=device, dtype=torch.float32)
    if p.dtype != torch.float32 or tuple(p.shape) != (N, 4) or not p.is_contiguous() or p.device != device:
        raise TypeError("%s: params_out must be a contiguous float32 [N, 4] on x's device" % op)
    p[:, :3] = params[:, :3].to(device=device, dtype=torch.float32)
    return p


class _DStage(NamedTuple):
    """A DiffAugment stage on D's input as the one-shot wrappers below see it: the draw and apply
    helpers read this and are the same code for every stage."""
    name: str           # of the wrappers in messages: <name>_draw, <name>_apply
    op: str             # Program.<op> / Program.<op>_bwd, recorded under the same names
    dtype: torch.dtype  # of the params rows [N, 4]
    check: str          # ops.reference's parser of a policy that is not yet the kernels' bitmask
    rows: object        # (op, params, params_out, N, device) -> the validated rows a probe / transpose reads
    gate_stream: int    # Philox stream of its gates (ops.reference.gate_masks)

    def mask(self, policy) -> int:
        from . import reference as R
        if isinstance(policy, int) and not isinstance(policy, bool):
            return policy
        return getattr(R, self.check)(policy).mask


_AUGMENT = _DStage("augment", "d_augment", torch.int32, "check_d_augment", _int_rows, 4)
_COLOR = _DStage("color", "d_color", torch.float32, "check_d_color", _color_rows, 5)


def _stage_draw(st: _DStage, x, seed, step, policy, out, params_out, p24, gates_out):
    op = st.name + "_draw"
    out = _aug_images(op, x, out)
    if not torch.is_tensor(step):
        v = int(step) & 0xFFFFFFFFFFFFFFFF  # (the counter's 64 bits as the int64 that holds them)
        step = torch.tensor([v - (1 << 64) if v >> 63 else v], dtype=torch.int64, device=x.device)
    _check_step(op, step)
    N, S, C = x.shape[0], x.shape[1], x.shape[3]
    if params_out is None:
        params_out = torch.empty(N, 4, device=x.device, dtype=st.dtype)
    if params_out.dtype != st.dtype or tuple(params_out.shape) != (N, 4) or not params_out.is_contiguous():
        raise TypeError("%s: params_out must be a contiguous %s [N, 4]" % (op, str(st.dtype).split(".")[-1]))
    prog = ext().Program(_ELEM_DT[x.dtype])
    px, po = (_p(x), _p(out)) if x.numel() else (0, 0)
    record, pp = getattr(prog, st.op), _p(params_out) if N else 0
    if p24 is None:
        record(st.op, px, po, pp, N, S, C, st.mask(policy), int(seed), _p(step))
        run(prog)
        return out, params_out
    state = _ada_state_arg(op, p24, x.device)
    if gates_out is None:
        gates_out = torch.empty(N, device=x.device, dtype=torch.int32)
    if gates_out.dtype != torch.int32 or tuple(gates_out.shape) != (N,) or not gates_out.is_contiguous():
        raise TypeError("%s: gates_out must be a contiguous int32 [N]" % op)
    record(st.op, px, po, pp, N, S, C, st.mask(policy), int(seed), _p(step), 0, _p(gates_out) if N else 0, _p(state))
    run(prog)
    return out, params_out, gates_out


def _stage_apply(st: _DStage, x, params, policy, transpose, out, params_out, gates):
    op = st.name + "_apply"
    out = _aug_images(op, x, out)
    N, S, C = x.shape[0], x.shape[1], x.shape[3]
    p = st.rows(op, params, params_out, N, x.device)
    prog = ext().Program(_ELEM_DT[x.dtype])
    px, po, pp = (_p(x), _p(out), _p(p)) if x.numel() else (0, 0, 0)
    # gates: integer [N], the recorded gate masks -- the gated kernel's probe / transpose
    pg = 0
    if gates is not None:
        gates = _gates_arg(op, gates, N, x.device)
        pg = _p(gates) if N else 0
    if transpose:
        getattr(prog, st.op + "_bwd")(st.op + "_bwd", px, po, pp, N, S, C, st.mask(policy), 0, pg)
    else:
        getattr(prog, st.op)(st.op, px, po, pp, N, S, C, st.mask(policy), 0, 0, 0, pg, 0)
    run(prog)
    return out


def augment_draw(x: torch.Tensor, seed: int, step, policy, out: Optional[torch.Tensor] = None,
                 params_out: Optional[torch.Tensor] = None, p24=None, gates_out: Optional[torch.Tensor] = None):
    """DiffAugment of x [N, S, S, C] as the training step runs it (d_augment_kernel): sample n draws
    (ty, tx, oy, ox) from the Philox stream (seed, step, 2). Returns (y, params int32 [N, 4]); policy: a
    DAugment, a policy list ("translation,cutout") or the kernels' bitmask. Oracle: ops.reference.augment
    over ops.reference.augment_params. p24 (an int, or the int32 [8] device state whose word 0 holds it):
    the gated kernel of adaptive augmentation -- returns (y, params, gates int32 [N]), gates the
    effective policy per sample (oracle: ops.reference.gate_masks on stream 4)."""
    return _stage_draw(_AUGMENT, x, seed, step, policy, out, params_out, p24, gates_out)


def augment_params(n: int, S: int, seed: int, step, device="cuda") -> torch.Tensor:
    """int32 [n, 4] = (ty, tx, oy, ox) as d_augment_kernel draws them for n samples of an S x S image
    from the Philox stream (seed, step, 2): the rows the kernel itself records, over a one-channel
    dummy image (oracle: ops.reference.augment_params)."""
    x = torch.zeros(int(n), int(S), int(S), 1, device=device, dtype=torch.bfloat16)
    return augment_draw(x, seed, step, 3)[1]


def augment_apply(x: torch.Tensor, params: torch.Tensor, policy, transpose: bool = False,
                  out: Optional[torch.Tensor] = None, gates: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DiffAugment of x [N, S, S, C] under given params [N, 4] = (ty, tx, oy, ox) (the kernel's probe
    entry), or with transpose=True its transposed gather, the backward (d_augment_bwd). Oracles:
    ops.reference.augment / augment_transpose."""
    return _stage_apply(_AUGMENT, x, params, policy, transpose, out, None, gates)


def color_draw(x: torch.Tensor, seed: int, step, policy, out: Optional[torch.Tensor] = None,
               params_out: Optional[torch.Tensor] = None, p24=None, gates_out: Optional[torch.Tensor] = None):
    """DiffAugment's color policy over x [N, S, S, C] as the training step runs it (d_color_kernel): sample
    n draws (b, s, c) from the Philox stream (seed, step, 3). Returns (y, params float32 [N, 4] = (b, s, c,
    Mx)); policy: a DColor, a policy list ("brightness,saturation,contrast") or the kernels' bitmask.
    Oracle: ops.reference.color_augment over ops.reference.color_params. p24: as ``augment_draw`` -- the
    gated kernel, returns (y, params, gates int32 [N]) (oracle: ops.reference.gate_masks on stream 5)."""
    return _stage_draw(_COLOR, x, seed, step, policy, out, params_out, p24, gates_out)


def color_params(n: int, seed: int, step, device="cuda") -> torch.Tensor:
    """float32 [n, 4] = (b, s, c, Mx) as d_color_kernel draws them for n samples from the Philox stream
    (seed, step, 3): the rows the kernel itself records, over a one-pixel dummy image of zeros (Mx = 0;
    oracle of the first three columns: ops.reference.color_params)."""
    x = torch.zeros(int(n), 1, 1, 1, device=device, dtype=torch.bfloat16)
    return color_draw(x, seed, step, 7)[1]


def color_apply(x: torch.Tensor, params: torch.Tensor, policy, transpose: bool = False,
                out: Optional[torch.Tensor] = None, params_out: Optional[torch.Tensor] = None,
                gates: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The color policy over x [N, S, S, C] under given params [N, 3 or 4] = (b, s, c[, Mx]) (the kernel's
    probe entry: it computes Mx itself and leaves it in column 3 of params_out, a float32 [N, 4], when
    one is given), or with transpose=True its transpose, the backward (d_color_bwd). Oracles:
    ops.reference.color_augment / color_augment_transpose."""
    return _stage_apply(_COLOR, x, params, policy, transpose, out, params_out, gates)


def gate_masks(n: int, seed: int, step, stream: int, p24, policy_mask: int, device="cuda") -> torch.Tensor:
    """int32 [n]: the gate masks the gated kernels record for n samples at p24 under `policy_mask` --
    stream 4: d_augment_kernel's (translation, cutout), stream 5: d_color_kernel's (brightness, saturation,
    contrast) -- over dummy images of zeros. Oracle: ops.reference.gate_masks."""
    for st in (_AUGMENT, _COLOR):
        if st.gate_stream == int(stream):
            x = torch.zeros(int(n), 1, 1, 1, device=device, dtype=torch.bfloat16)
            return _stage_draw(st, x, seed, step, int(policy_mask), None, None, p24, None)[2]
    raise ValueError("gate_masks: stream must be 4 (translation / cutout) or 5 (color), got %r" % (stream,))


def ada_update(state: torch.Tensor, real_logits: torch.Tensor, thr: float, target_n: int, delta24: int,
               interval: int) -> torch.Tensor:
    """One step of the adaptive-augmentation controller (ada_update_kernel), in place on state int32 [8] =
    (p24, acc, cnt, r_acc, windows, 0, 0, 0), from the fp32 real logits [B]. Oracle: ops.reference.ada_update."""
    if state.dtype != torch.int32 or state.numel() != 8 or not state.is_contiguous():
        raise TypeError("ada_update: state must be a contiguous int32 [8]")
    if real_logits.dtype != torch.float32 or real_logits.dim() != 1 or not real_logits.is_contiguous():
        raise TypeError("ada_update: real_logits must be a contiguous float32 [B]")
    prog = ext().Program()
    prog.ada_update("ada_update", _p(real_logits) if real_logits.numel() else 0, real_logits.numel(), _p(state),
                    float(thr), int(target_n), int(delta24), int(interval))
    run(prog)
    return state


def adam_(w: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, powers: torch.Tensor, lr: float,
          beta1: float, beta2: float, eps: float, gscale: float = 1.0, advance_powers: bool = True,
          lr_sched=None, step: Optional[torch.Tensor] = None) -> None:
    """TF-Adam over w (fp32; g fp32, or bf16: the all-reduced wire image). lr_sched / step: lr times
    the schedule's factor at step[0], evaluated in the kernel."""
    prog = ext().Program()
    kw = _lr_kw(lr_sched, step, "adam_")
    if g.dtype == torch.bfloat16:
        prog.adam_bf("adam", _p(w), 0, 0, _p(m), _p(v), _p(powers), w.numel(), lr, beta1, beta2, eps, gscale, 0, 0,
                     _p(g), **kw)
    else:
        prog.adam("adam", _p(w), _p(g), _p(m), _p(v), _p(powers), w.numel(), lr, beta1, beta2, eps, gscale, 0, **kw)
    if advance_powers:
        prog.step_end("powers", _p(powers), 0, beta1, beta2, 0.0, 0.0, 0, 0)
    run(prog)


def adam1_max_blocks() -> int:
    """Grid cap of the D sub-step's one-launch update (larger buffers grid-stride)."""
    return int(ext().ADAM1_MAX_BLOCKS)


def adam1_(w: torch.Tensor, wbf: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
           powers: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, gscale: float = 1.0,
           lr_sched=None, step: Optional[torch.Tensor] = None) -> None:
    """The D sub-step's update in one launch: TF-Adam over w (fp32, numel % 4 == 0), its 16-bit mirror
    wbf, and powers *= (beta1, beta2) once every block has read them. lr_sched / step: as adam_."""
    if wbf.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("adam1_: the mirror must be bfloat16 or float16")
    if any(t.dtype != torch.float32 for t in (w, g, m, v, powers)):
        raise TypeError("adam1_: w, g, m, v and powers must be float32")
    n = w.numel()
    if n % 4 or any(t.numel() != n for t in (wbf, g, m, v)) or powers.numel() != 2:
        raise ValueError("adam1_: equal sizes, numel % 4 == 0, two powers")
    prog = ext().Program(int(wbf.dtype == torch.float16))
    prog.adam1("adam1", _p(w), _p(wbf), _p(g), _p(m), _p(v), _p(powers), n, lr, beta1, beta2, eps, gscale, 0,
               **_lr_kw(lr_sched, step, "adam1_"))
    run(prog)


def gan_loss_id(kind: str, label_smooth: float = 0.0) -> int:
    """Objective id of the loss / head kernels for a validated (name, label_smooth) pair."""
    from .reference import check_gan_loss
    return GAN_LOSS_IDS[check_gan_loss(kind, label_smooth)[0]]


def gan_loss(logits: torch.Tensor, kind: str = "bce", label_smooth: float = 0.0,
             ls: Optional[torch.Tensor] = None):
    """The stand-alone loss kernel on fp32 logits [2B] (real rows first): (losses[4] = d_loss_real,
    d_loss_fake, g_loss, d_loss; dl_d[2B]; dl_g[B]; prob[2B] = sigmoid). ls = fp16 loss-scale state:
    the seeds carry ls[0], the losses do not."""
    if logits.dtype != torch.float32 or logits.dim() != 1 or logits.numel() % 2 or not logits.numel():
        raise TypeError("gan_loss: logits must be a float32 vector of 2B elements")
    obj = gan_loss_id(kind, label_smooth)
    B = logits.numel() // 2
    out, dl_d, dl_g, prob = (torch.empty(n, device=logits.device, dtype=torch.float32) for n in (4, 2 * B, B, 2 * B))
    prog = ext().Program()
    prog.gan_loss("gan_loss", _p(logits), B, _p(out), _p(dl_d), _p(dl_g), _p(prob), 0, _p(ls), obj,
                  float(label_smooth))
    run(prog)
    return out, dl_d, dl_g, prob


def g_topk(logits: torch.Tensor, dl_g: torch.Tensor, k_or_sched, kind: str = "bce",
           step: Optional[torch.Tensor] = None, out=None):
    """The top-k kernel on the fp32 fake logits [B] and the all-sample seed dl_g [B] (as gan_loss wrote it,
    loss scale included): (dl_g_k float32[B], sel int32[B], info float32[4] = g_loss_topk, threshold, B / k,
    k). k_or_sched: an int k, or (kmin, nsteps) evaluated at the device counter step[0] (int64). out: the
    three output buffers, when the caller brings its own. Oracle: ops.reference.topk_*."""
    if logits.dtype != torch.float32 or logits.dim() != 1 or dl_g.dtype != torch.float32 or dl_g.shape != logits.shape:
        raise TypeError("g_topk: logits and dl_g must be float32 vectors of B elements")
    if not (logits.is_contiguous() and dl_g.is_contiguous()):
        raise ValueError("g_topk: logits and dl_g must be contiguous")
    from .reference import check_gan_loss
    obj = GAN_LOSS_IDS[check_gan_loss(kind)[0]]
    B = logits.numel()
    if isinstance(k_or_sched, int):  # a fixed k: the end of a one-step anneal
        kmin, nsteps = k_or_sched, 1
        if step is None:
            step = torch.ones(1, device=logits.device, dtype=torch.int64)
    else:
        kmin, nsteps = k_or_sched
        if step is None:
            raise TypeError("g_topk: a (kmin, nsteps) schedule needs the step counter")
    _check_step("g_topk", step)
    if out is None:
        out = (torch.empty(B, device=logits.device, dtype=torch.float32),
               torch.empty(B, device=logits.device, dtype=torch.int32),
               torch.empty(4, device=logits.device, dtype=torch.float32))
    dl_g_k, sel, info = out
    if dl_g_k.dtype != torch.float32 or sel.dtype != torch.int32 or info.dtype != torch.float32 or \
            dl_g_k.numel() != B or sel.numel() != B or info.numel() != 4:
        raise TypeError("g_topk: out must be (float32[B], int32[B], float32[4])")
    prog = ext().Program()
    prog.g_topk("g_topk", _p(logits) if B else 0, _p(dl_g) if B else 0, _p(dl_g_k) if B else 0, _p(sel) if B else 0,
                _p(info), B, int(kmin), int(nsteps), _p(step), obj)
    run(prog)
    return dl_g_k, sel, info


def topk_k(steps: torch.Tensor, B: int, kmin: int, nsteps: int) -> torch.Tensor:
    """k(t) of the top-k anneal at each step value, int64[N] -> int32[N], from the device function the
    top-k kernel evaluates (dcg::topk_k)."""
    if steps.dtype != torch.int64:
        raise TypeError("topk_k: steps must be int64")
    steps = steps.contiguous()
    out = torch.empty(steps.shape, device=steps.device, dtype=torch.int32)
    prog = ext().Program()
    prog.topk_k("topk_k", _p(steps) if steps.numel() else 0, _p(out), steps.numel(), int(B), int(kmin), int(nsteps))
    run(prog)
    return out


def ema_max_blocks() -> int:
    """Grid cap of the streaming EMA kernel (larger buffers grid-stride)."""
    return int(ext().EMA_MAX_BLOCKS)


def ema_(s: torch.Tensor, sbf: Optional[torch.Tensor], w: torch.Tensor, decay: float, step: torch.Tensor,
         step_bias: int = 0, ls: Optional[torch.Tensor] = None) -> None:
    """In place s -= (1 - d_t)(s - w), d_t = min(decay, (1 + t) / (10 + t)), t = step[0] + step_bias
    (device int64 counter); sbf (optional) receives s in its 16-bit dtype; ls = fp16 loss-scale
    state [scale, overflow, good steps]: a set overflow flag leaves s and sbf untouched."""
    if s.dtype != torch.float32 or w.dtype != torch.float32 or step.dtype != torch.int64:
        raise TypeError("ema_: s, w must be float32 and step int64")
    if w.numel() != s.numel() or (sbf is not None and sbf.numel() != s.numel()):
        raise ValueError("ema_: s, sbf and w must have the same number of elements")
    dt = 0
    if sbf is not None:
        if sbf.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError("ema_: the mirror must be bfloat16 or float16")
        dt = int(sbf.dtype == torch.float16)
    prog = ext().Program(dt)
    prog.ema("ema", _p(s), _p(sbf), _p(w), s.numel(), float(decay), _p(step), int(step_bias), _p(ls), 0)
    run(prog)


# --------------------------------------------------------------------------- spectral norm (D)
def sn_plan(K: int, Cout: int) -> Tuple[int, int, int, int, int]:
    """(row blocks, rows per block, column tiles, streaming blocks, workspace floats) of the
    spectral-norm kernels for a [K, Cout] matrix."""
    return tuple(int(x) for x in ext().sn_plan(int(K), int(Cout)))


def sn_workspace(K: int, Cout: int, device) -> torch.Tensor:
    return torch.zeros(sn_plan(K, Cout)[4], dtype=torch.float32, device=device)


_SN_BUILDS = {"bf16": 0, "fp16": 1, "fp32": 2}


def _sn_tuples(what, mats, hats, grads, build):
    """Program dtype + the descriptor tuples of ``Program.sn_*`` from (W, u, v, sigma, ws) rows."""
    if build not in _SN_BUILDS:
        raise ValueError("%s: build must be one of %s" % (what, sorted(_SN_BUILDS)))
    dt = _SN_BUILDS[build]
    edt = {0: torch.bfloat16, 1: torch.float16, 2: torch.float32}[dt]
    out = []
    for i, (W, u, v, sigma, ws) in enumerate(mats):
        if W.dim() != 2:
            raise ValueError("%s: W must be [K, Cout]" % what)
        K, C = W.shape
        if K == 0 or C == 0:
            raise ValueError("%s: K and Cout must be positive" % what)
        for t in (W, u, v, sigma, ws):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError("%s: W, u, v, sigma and ws must be contiguous float32" % what)
        if u.numel() != C or v.numel() != K or sigma.numel() != 1 or ws.numel() < sn_plan(K, C)[4]:
            raise ValueError("%s: u [Cout], v [K], sigma [1], ws [sn_plan(K, Cout)[4]]" % what)
        hat = hats[i] if hats is not None else None
        grad = grads[i] if grads is not None else None
        hf = 0
        if hat is not None:
            if hat.dtype not in (torch.float32, edt) or hat.numel() != K * C or not hat.is_contiguous():
                raise TypeError("%s: the normalised copy must be float32 or %s, K * Cout elements" % (what, edt))
            hf = int(hat.dtype == torch.float32)
        if grad is not None and (grad.dtype != torch.float32 or grad.numel() != K * C or not grad.is_contiguous()):
            raise TypeError("%s: the gradient must be contiguous float32, K * Cout elements" % what)
        out.append((_p(W), _p(u), _p(v), _p(sigma), _p(ws), _p(hat), hf, _p(grad), K, C))
    return dt, out


def sn_power_(mats, hats, ls: Optional[torch.Tensor] = None, build: str = "fp32") -> None:
    """One power-iteration step per matrix, in place: mats = [(W [K, Cout], u, v, sigma, ws)], all
    fp32; v = W u / max(|W u|, eps), sigma = max(|W^T v|, eps), u = W^T v / sigma, and hats[i]
    (fp32, or the 16-bit dtype of ``build``) receives W * (1 / sigma). ls = fp16 loss-scale state: a
    set overflow flag leaves everything untouched. 4 launches for all matrices (at most 8)."""
    dt, tup = _sn_tuples("sn_power_", mats, hats, None, build)
    prog = ext().Program(dt)
    prog.sn_power("sn_power", tup, _p(ls), 0)
    run(prog)


def sn_apply_(mats, hats, build: str = "fp32") -> None:
    """hats[i] = W * (1 / sigma) from the stored sigma (no iteration): 1 launch."""
    dt, tup = _sn_tuples("sn_apply_", mats, hats, None, build)
    prog = ext().Program(dt)
    prog.sn_apply("sn_apply", tup, 0)
    run(prog)


def sn_project_(mats, grads, build: str = "fp32") -> None:
    """In place grads[i] = (G - <G, W> / sigma * v u^T) / sigma with the stored u, v, sigma: the
    gradient of W / sigma(W) projected back to W. 2 launches for all matrices."""
    dt, tup = _sn_tuples("sn_project_", mats, None, grads, build)
    prog = ext().Program(dt)
    prog.sn_project("sn_project", tup, 0)
    run(prog)
