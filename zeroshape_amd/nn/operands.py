"""The derived weight operands of the training path, and their one owner.

A training GEMM never reads a Parameter: it reads a packed copy (zs_pack_conv_weight), made from the standardised weight for
StdConv layers, and under optim.amp the packed copy's fp16 halves.  Parameters stay in the reference's torch layout and the
derived forms are refreshed on the GPU when a weight changes, so optimiser steps need no host work.  Only this module knows
how an operand is keyed, stamped, refreshed and dropped: SWITCHES says which forms are kept current, CACHE holds the records
and the per-device launch tables, nn/autograd.py asks CACHE for the tensor a launch reads.
"""
import os
import weakref

import numpy as np
import torch

from .. import _lib
from .ops import CONV_F16X3, CONV_IN_DILATE2, CONV_W_PRESPLIT      # ZS_CONV_* flags of zs_conv2d_nhwc

# Bumped whenever parameters are updated through raw pointers (the fused optimiser): tensor
# ._version does not see those writes, so every pack cache also keys on this counter.
GENERATION = [0]


def bump_generation():
    GENERATION[0] += 1


class Switches(object):
    """Which arithmetic the training GEMMs use, and with it which forms of a packed operand are kept current."""

    def __init__(self, env=os.environ):
        # Arithmetic of the FORWARD convolutions / linear layers of the training path: "f32" (default) or
        # "f16x3" = split-fp16 (opt-in: 15.4 -> 14.4 ms forward per step at batch 4, but the 1e-6 forward
        # differences are amplified by the batch-statistics BatchNorms to ~2e-3 relative in some gradients,
        # beyond this repository's gradient parity bar).
        self.forward = env.get("ZS_TRAIN_FWD_PRECISION", "f32")
        # Data gradients (dx = dy * W^T through the same convolution engine).  "f16x3" needs the incoming gradients inside
        # fp16's range: the Runner multiplies the loss by a dynamic power of two (optim.LossScaler, torch's GradScaler
        # rules) and the optimiser divides it out, an overflow (inf / nan in any gradient) skips the step and halves the
        # scale.  Weight gradients stay exact fp32 (they sum over every pixel of the batch).
        self.backward = env.get("ZS_TRAIN_BWD_PRECISION", "f32")
        # ONE launch right behind the re-pack splits every registered operand (zs_conv2d_presplit_weight_multi), so every
        # split-fp16 kernel reads ready halves and the 40 per-layer split launches go.  Round 3 measured this SLOWER (29.75 ->
        # 30.1 ms: the small-tile kernels are latency-bound and the split of 192 M parameters moves 1.5 GB); since round 4 the
        # few-row pointwise layers with a split operand take the streaming GEMM kernel (csrc/nn_gemm_stream.hip; batch 4 = 788
        # token rows) and it pays: optim.amp step 29.71 -> 28.87 ms on the same box.  ZS_TRAIN_PRESPLIT_ALL=0: only the
        # >= 192-tile layers, per layer.
        self.presplit_all = env.get("ZS_TRAIN_PRESPLIT_ALL", "1") != "0"
        self.inline_split = env.get("ZS_TRAIN_INLINE_SPLIT", "1") != "0"      # A/B switch
        # optim.amp: layers large enough for the LDS-DMA GEMM kernel or the 3x3 input-patch kernels (>= 192 tiles of 128 x 128,
        # channels a multiple of 16, no input affine) get their packed operand split into fp16 halves once per optimiser step
        # (zs_conv2d_presplit_weight), which is what those kernels consume; the other layers split on the fly as before.
        self.presplit_min_tiles = int(env.get("ZS_TRAIN_PRESPLIT_MIN_TILES", "192"))

    def amp_splits_operands(self):
        return self.presplit_all and (self.forward == "f16x3" or self.backward == "f16x3")

    def inline_split_mode(self):
        """0: re-pack only.  1: the re-pack also writes the fp16 halves.  2: ... and leaves the fp32 operands of those entries
        alone (forward AND data gradients read the halves: nothing reads the fp32 form until the precision changes, which
        bumps the generation and so re-packs everything)."""
        if not (self.inline_split and self.amp_splits_operands()):
            return 0
        return 2 if self.forward == "f16x3" and self.backward == "f16x3" else 1

    def operand_forms(self):
        return (bool(self.presplit_all), bool(self.inline_split), self.forward == "f16x3", self.backward == "f16x3")


SWITCHES = Switches()


def set_forward_precision(p):
    """"f32" | "f16x3": arithmetic of the forward convolutions / linear layers under autograd (optim.amp selects
    "f16x3": the 16-bit matrix pipe with split operands, fp32 accumulation)."""
    if p not in ("f32", "f16x3"):
        raise ValueError("forward precision must be 'f32' or 'f16x3', got %r" % (p,))
    if p != SWITCHES.forward:
        GENERATION[0] += 1      # operands re-packed under the other setting may hold only the form that one reads
    SWITCHES.forward = p


def set_backward_precision(p):
    if p not in ("f32", "f16x3"):
        raise ValueError("data-gradient precision must be 'f32' or 'f16x3', got %r" % (p,))
    if p != SWITCHES.backward:
        GENERATION[0] += 1
    SWITCHES.backward = p


def stamp(w):
    # ... and the switches that decide WHICH forms of a packed operand are kept current (in mode 2 the re-pack
    # writes only the fp16 halves; a tool or test that flips presplit_all / inline_split at run time must find every record
    # stale, not a fresh-looking stamp over an fp32 operand nobody has rewritten since)
    return (w.data_ptr(), w._version, GENERATION[0], SWITCHES.operand_forms())


def weights_stamp(tensors):
    """ "Have these weights changed": the key of everything derived from a set of parameters / buffers outside this cache."""
    return (GENERATION[0],) + tuple((t.data_ptr(), t._version) for t in tensors)


def ceil4(n):
    return (n + 3) // 4 * 4


class _StdRec(object):
    """A timm StdConv2d weight standardised into a persistent buffer; `stamp` is that of the weight it was made from."""
    __slots__ = ("ref", "eps", "buffer", "stamp")


class _PackRec(object):
    # split / split_stamp: the operand's fp16 halves (optim.amp) and the stamp of the pack they were made from - a re-pack
    # (in-place weight update, load_state_dict, optimiser step) moves `stamp` and so invalidates the split with it; the
    # buffer dies with the record (a cache keyed by packed.data_ptr() + generation served stale weights)
    # inline_split: the multi re-pack writes this operand's halves itself (zs_pack_conv_weight_multi_split)
    __slots__ = ("ref", "key", "packed", "stamp", "dims", "split", "split_stamp", "inline_split")


def _pack_dims(w, cin, dgrad):
    cout, cintot = w.shape[0], w.shape[1]
    kh, kw = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    taps = kh * kw
    kc, n = (ceil4(cout), cin) if dgrad else (ceil4(cin), cout)
    return cout, cintot, kh, kw, taps, (taps * kc + 15) // 16 * 16, (n + 127) // 128 * 128


def _i64(values, device):
    return torch.tensor(values, dtype=torch.int64).to(device)


class OperandCache(object):
    """Standardised weights and packed GEMM operands in persistent buffers, re-packed for ALL layers in one launch.  Records
    die with their weight (weakref callbacks), so every walk over a registry goes over a copy."""

    def __init__(self):
        self.std = {}       # id(weight) -> _StdRec
        self.packs = {}     # (id(weight), cin0, cin, dgrad, std_eps) -> _PackRec
        self.epoch = 0      # bumped whenever `packs` gains or loses a record
        self.fast = {}      # device -> dict(epoch, generation, recs, ptrs): the last complete re-pack, for its replay
        # (kind, device) -> (signature, launch table ...) of the multi launches: "std" standardize_all, "pack" the re-pack,
        # "split" the split behind it.  A table keeps its split buffers alive: a captured hipGraph holds their addresses.
        self.tables = {}

    def clear(self):
        self.packs.clear()
        self.std.clear()
        self.tables.clear()
        self.fast.clear()
        self.epoch += 1

    def drop(self, key):
        if self.packs.pop(key, None) is not None:
            self.epoch += 1

    def _table(self, kind, device, sig, build):
        """The cached device table of a multi launch, rebuilt by build() when the set of entries (`sig`) changed."""
        cached = self.tables.get((kind, device))
        if cached is None or cached[0] != sig:
            if torch.cuda.is_current_stream_capturing():
                # the table would travel by a host-to-device copy from pageable memory: not capturable (the graph
                # would keep the host address).  refresh_packs() before the capture builds it.
                raise RuntimeError("the set of %s changed inside a stream capture; call "
                                   "zeroshape_amd.nn.autograd.refresh_packs(device) before capturing"
                                   % ("standardised weights" if kind == "std" else "packed operands"))
            cached = self.tables[(kind, device)] = (sig,) + tuple(build())
        return cached

    # ---- standardised weights ----
    def _std_rec(self, weight, eps):
        rec = self.std.get(id(weight))
        if rec is None or rec.ref() is not weight or rec.eps != float(eps):
            rec = self.std[id(weight)] = _StdRec()
            rec.ref = weakref.ref(weight, lambda _r, k=id(weight): self.std.pop(k, None))
            rec.eps, rec.buffer, rec.stamp = float(eps), torch.empty_like(weight.detach()), None
        return rec

    def standardize(self, weight, eps):
        """timm StdConv2d weight standardisation of a Parameter, refreshed when the weight changes."""
        rec = self._std_rec(weight, eps)
        if rec.stamp != stamp(weight):
            w = weight.detach()
            with _lib.on(w.device):
                _lib.check(_lib.load().zs_standardize_weight(_lib.ptr(w), _lib.ptr(rec.buffer), w.shape[0], w[0].numel(),
                                                             float(eps), _lib.current_stream_ptr(w.device)),
                           "zs_standardize_weight")
            rec.stamp = stamp(weight)
        return rec.buffer

    def standardize_all(self, pairs):
        """standardize() for a list of (weight, eps) in ONE launch (zs_standardize_weight_multi): the stale ones of the list go
        through a cached device table - after an optimiser step that is every StdConv weight of the model (52 launches before)."""
        todo, seen = [], set()
        for weight, eps in pairs:
            rec = self._std_rec(weight, eps)
            if rec.stamp != stamp(weight) and id(weight) not in seen:
                seen.add(id(weight))
                todo.append((weight, rec))
        if not todo:
            return
        if len(todo) == 1:
            self.standardize(todo[0][0], todo[0][1].eps)
            return
        device = todo[0][0].device
        sig = tuple((w.data_ptr(), rec.buffer.data_ptr(), w.shape[0], w[0].numel(), rec.eps) for w, rec in todo)

        def build():
            dt = np.dtype([("w", "<u8"), ("out", "<u8"), ("rows", "<i4"), ("n", "<i4"), ("eps", "<f4"), ("pad", "<i4")])
            assert dt.itemsize == 32
            tab = np.zeros(len(sig), dt)
            prefix, total = [], 0
            for i, e in enumerate(sig):
                tab[i] = e + (0,)
                prefix.append(total)
                total += e[2]
            return (torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(device),
                    torch.tensor(prefix, dtype=torch.int32).to(device), len(sig), total)

        _, tab_d, pre_d, n, total = self._table("std", device, sig, build)
        with _lib.on(device):
            _lib.check(_lib.load().zs_standardize_weight_multi(_lib.ptr(tab_d), _lib.ptr(pre_d), n, total,
                                                               _lib.current_stream_ptr(device)), "zs_standardize_weight_multi")
        for w, rec in todo:
            rec.stamp = stamp(w)

    # ---- packed operands ----
    def pack(self, weight, cin0, cin, dgrad, std_eps=None):
        """The record of the packed GEMM operand (`.packed`) of `weight` (torch layout [Cout, CinTot(, kh, kw)], optionally
        standardised first) for the forward product (dgrad=False) or the data gradient.  Operands live
        in persistent buffers; the first use of a layer packs it alone, afterwards a stale operand
        triggers ONE launch that re-packs every registered operand whose weight changed (the state after
        an optimiser step), instead of ~450 small launches per training step."""
        key = (id(weight), cin0, cin, bool(dgrad), std_eps)
        rec = self.packs.get(key)
        if rec is not None and rec.ref() is weight:
            if rec.stamp != stamp(weight):
                self.refresh(weight.device)
            return rec
        w = self.standardize(weight, std_eps) if std_eps is not None else weight.detach()
        dims = _pack_dims(w, cin, dgrad)
        cout, cintot, kh, kw, taps, K16, NPad = dims
        rec = _PackRec()
        rec.ref = weakref.ref(weight, lambda _r, k=key: self.drop(k))
        rec.key, rec.dims = key, dims
        rec.packed = torch.empty(K16 * NPad, dtype=torch.float32, device=w.device)
        rec.split, rec.split_stamp, rec.inline_split = None, None, False
        with _lib.on(w.device):
            _lib.check(_lib.load().zs_pack_conv_weight(_lib.ptr(w), _lib.ptr(rec.packed), cout, cin, cin0, cintot, kh, kw,
                                                       1 if dgrad else 0, _lib.current_stream_ptr(w.device)),
                       "zs_pack_conv_weight")
        rec.stamp = stamp(weight)
        self.packs[key] = rec
        self.epoch += 1
        return rec

    def refresh(self, device):
        """Re-pack every registered operand on `device` whose weight changed, then (optim.amp) split every operand."""
        self.repack(device)
        if SWITCHES.amp_splits_operands():
            self._split_all(device)

    def replayable(self, device):
        """The state after an optimiser step (every step of a training run): the same records as the last time, all of
        them stale because the generation moved, the same weight pointers.  -> [(record, weight)] of that re-pack, or None."""
        fast = self.fast.get(device)
        if fast is None or fast["epoch"] != self.epoch or fast["generation"] == GENERATION[0]:
            return None
        live = [(rec, rec.ref()) for rec in fast["recs"]]
        return live if all(w is not None and w.data_ptr() == ptr for (rec, w), ptr in zip(live, fast["ptrs"])) else None

    def _launch_multi_pack(self, device, table, recs):
        """One launch over the re-pack table; then the records carry the new stamps, and the halves the launch wrote itself
        are those of the current operand."""
        sig, tab_d, ce_d, cs_d, n, split_d, _splits = table
        lib = _lib.load()
        with _lib.on(device):
            if split_d is None:
                _lib.check(lib.zs_pack_conv_weight_multi(_lib.ptr(tab_d), _lib.ptr(ce_d), _lib.ptr(cs_d), n,
                                                         _lib.current_stream_ptr(device)), "zs_pack_conv_weight_multi")
            else:
                _lib.check(lib.zs_pack_conv_weight_multi_split(_lib.ptr(tab_d), _lib.ptr(ce_d), _lib.ptr(cs_d), n,
                                                               _lib.ptr(split_d), 1 if sig[-1] == 2 else 0,
                                                               _lib.current_stream_ptr(device)),
                           "zs_pack_conv_weight_multi_split")
        for rec, w in recs:
            rec.stamp = stamp(w)
            if split_d is not None and rec.inline_split and rec.split is not None:
                rec.split_stamp = rec.stamp

    def repack(self, device):
        """Re-pack every registered operand on `device` whose weight changed, in ONE launch."""
        # Replay the last complete re-pack - standardise the StdConv weights into their persistent buffers, launch over the
        # cached table - without rebuilding the entry list.
        live = self.replayable(device)
        if live is not None:
            self.standardize_all([(w, rec.key[4]) for rec, w in live if rec.key[4] is not None])
            table = self.tables[("pack", device)]
            if table[0][-1] == SWITCHES.inline_split_mode():
                self._launch_multi_pack(device, table, live)
                self.fast[device]["generation"] = GENERATION[0]
                return
        recs = []
        # iterate over a copy: a weight collected while the loop allocates fires its weakref callback (drop) mid-loop
        for key, rec in self.packs.copy().items():
            w = rec.ref()
            if w is None:
                self.drop(key)
            elif w.device == device and rec.stamp != stamp(w):
                recs.append((rec, w))
        if not recs:
            return
        complete = len(recs) == sum(1 for rec in self.packs.copy().values()
                                    if rec.ref() is not None and rec.ref().device == device)
        lib = _lib.load()
        entries = []
        self.standardize_all([(w, rec.key[4]) for rec, w in recs if rec.key[4] is not None and w.device == device])
        for rec, w in recs:
            _, cin0, cin, dgrad, std_eps = rec.key
            src = self.standardize(w, std_eps) if std_eps is not None else w.detach()
            cout, cintot, kh, kw, taps, K16, NPad = rec.dims
            entries.append((src.data_ptr(), rec.packed.data_ptr(), cout, cin, cin0, cintot * taps, taps, 1 if dgrad else 0,
                            K16, NPad))
        mode = SWITCHES.inline_split_mode()

        def build():
            dt = np.dtype([("src", "<u8"), ("dst", "<u8")] + [(n, "<i4") for n in ("Cout", "Cin", "cin0", "ld", "taps", "dgrad",
                                                                                 "K16", "NPad")])
            assert dt.itemsize == 48
            tab = np.zeros(len(entries), dt)
            ce, cs = [], []
            for i, e in enumerate(entries):
                tab[i] = e
                n_chunks = lib.zs_pack_entry_chunks(e[2], e[3], e[6], e[7], e[8], e[9])
                _lib.check(1 if n_chunks > 0 else 0, "zs_pack_entry_chunks")
                starts = np.arange(n_chunks, dtype=np.uint64)
                ce.append(np.full(len(starts), i, np.int32))
                cs.append(starts)
            ce, cs = np.concatenate(ce), np.concatenate(cs)
            # optim.amp: the halves of every operand whose tiles hold whole K = 16 groups leave the same launch (split_d: one
            # pointer per entry, 0 = the operand is split by _split_all's launch behind this one)
            split_d, splits = None, []
            if mode:
                ptrs = []
                for (rec, _), e in zip(recs, entries):
                    rec.inline_split = bool(lib.zs_pack_entry_inline_split(e[2], e[3], e[6], e[7]))
                    if rec.inline_split:
                        if rec.split is None or rec.split.numel() != rec.packed.numel() or rec.split.device != device:
                            rec.split = torch.empty_like(rec.packed)
                        ptrs.append(rec.split.data_ptr())
                        splits.append(rec.split)
                    else:
                        ptrs.append(0)
                split_d = _i64(ptrs, device)
            else:
                for rec, _ in recs:
                    rec.inline_split = False
            return (torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(device), torch.from_numpy(ce).to(device),
                    torch.from_numpy(cs.view(np.int64)).to(device), len(ce), split_d, splits)

        self._launch_multi_pack(device, self._table("pack", device, tuple(entries) + (mode,), build), recs)
        if complete:
            self.fast[device] = dict(epoch=self.epoch, generation=GENERATION[0], recs=[rec for rec, _ in recs],
                                     ptrs=[w.data_ptr() for _, w in recs])
        else:
            self.fast.pop(device, None)

    # ---- fp16 halves (optim.amp) ----
    def _split_all(self, device):
        """Split every registered packed operand on `device` (call right after they were re-packed)."""
        recs = [rec for rec in self.packs.copy().values() if rec.ref() is not None and rec.packed.device == device and
                not (rec.inline_split and rec.split is not None and rec.split_stamp == rec.stamp)]   # (split by the re-pack itself)
        if not recs:
            return
        sig = tuple((rec.packed.data_ptr(), rec.packed.numel()) for rec in recs)

        def build():
            splits, src, dst, cps, prefix, tot = [], [], [], [], [0], 0
            for rec in recs:
                K16, NPad = rec.dims[5], rec.dims[6]
                sp = rec.split
                if sp is None or sp.numel() != rec.packed.numel() or sp.device != device:
                    sp = torch.empty_like(rec.packed)
                splits.append(sp)
                src.append(rec.packed.data_ptr()); dst.append(sp.data_ptr()); cps.append(NPad)
                tot += K16 // 16 * 2 * NPad
                prefix.append(tot)
            return (_i64(src, device), _i64(dst, device), torch.tensor(cps, dtype=torch.int32).to(device),
                    _i64(prefix, device), len(recs), tot, splits)

        _, src_d, dst_d, cp_d, pre_d, n, tot, splits = self._table("split", device, sig, build)
        with _lib.on(device):
            _lib.check(_lib.load().zs_conv2d_presplit_weight_multi(_lib.ptr(src_d), _lib.ptr(dst_d), _lib.ptr(cp_d),
                                                                   _lib.ptr(pre_d), n, tot, _lib.current_stream_ptr(device)),
                       "zs_conv2d_presplit_weight_multi")
        for rec, sp in zip(recs, splits):
            rec.split, rec.split_stamp = sp, rec.stamp

    def split_of(self, rec):
        """The operand's current fp16 halves, or None (never split, or split from an older pack)."""
        if rec.split is not None and rec.split_stamp == rec.stamp and rec.split.numel() == rec.packed.numel():
            return rec.split
        return None

    def presplit(self, rec, C, Co, kh, kw):
        """The operand's fp16 halves, split now (this layer alone) unless they are current."""
        split = self.split_of(rec)
        if split is None:
            packed = rec.packed
            split = rec.split if rec.split is not None and rec.split.numel() == packed.numel() else torch.empty_like(packed)
            with _lib.on(packed.device):
                _lib.check(_lib.load().zs_conv2d_presplit_weight(_lib.ptr(packed), _lib.ptr(split), C, Co, kh, kw,
                                                                 _lib.current_stream_ptr(packed.device)),
                           "zs_conv2d_presplit_weight")
            rec.split, rec.split_stamp = split, rec.stamp
        return split

    def operand(self, rec, flags, rows, C, Co, kh, kw, in_scale, in_shift):
        """-> (tensor, flags) a convolution launch over `rows` output pixels reads `rec` through: the fp32 pack, or for a
        split-fp16 launch its halves + CONV_W_PRESPLIT when they are current or the layer is worth splitting on its own."""
        if flags & CONV_F16X3:
            split = self.split_of(rec) if SWITCHES.amp_splits_operands() else None
            if split is not None:
                return split, flags | CONV_W_PRESPLIT      # split with every other operand right after the re-pack
            if not (flags & CONV_IN_DILATE2) and C % 16 == 0 and in_scale == 1.0 and in_shift == 0.0 and \
                    -(-rows // 128) * -(-Co // 128) >= SWITCHES.presplit_min_tiles:
                return self.presplit(rec, C, Co, kh, kw), flags | CONV_W_PRESPLIT
        return rec.packed, flags


CACHE = OperandCache()


def refresh_packs(device):
    """Re-pack every registered operand on `device` now (and leave the launch table of that set cached): what a
    stream capture of a training step must do first, so that the re-pack inside the capture finds its table."""
    bump_generation()
    CACHE.refresh(torch.device(device) if not isinstance(device, torch.device) else device)
