"""Observability / inference helpers of the HIP engine (mixin of ``hip_engine.HipEngine``): views
of the last step's tensors, on-device TensorBoard summaries, the EMA-BN sampler
(``distriubted_model.py:131-153``), sample-time losses (``image_train.py:181-184``) and the
launch / placement accounting behind ``--log_device_placement`` and bench.py's kernel count. None
of it runs inside the training step."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional

import torch

from ..models.config import same_pads
from ..ops import hip as H
from ..ops import reference as R

RELU, TANH = 1, 3


def _p(t) -> int:
    return 0 if t is None else int(t.data_ptr())


class HipEngineAux:
    def activations(self) -> "Dict[str, torch.Tensor]":
        """Views of the last step's tensors for summaries (no extra compute)."""
        B = self.B
        a = OrderedDict()
        a["z"] = self.z
        a["d"] = self.prob[:B]
        a["d_"] = self.prob[B:]
        a["G"] = self.fake
        a["g_h0_relu"] = self.g_h0
        for L in self.gl[:-1]:
            a[L.name + "_relu"] = self.g_a[L.name]
        a[self.gl[-1].name] = self.fake
        for L in self.dl:
            a[L.name] = self.d_a[L.name][:B]
        a[self.cfg.d_lin_name] = self.logits[:B]
        return a

    # ------------------------------------------------------------------ device-side summaries
    def device_summaries(self) -> "OrderedDict[str, object]":
        """Zero fraction + TF-bucket histogram statistics of every summarised tensor, computed on
        the device (summary.hip) in ONE program; only the per-tensor statistics rows (a few KB
        each) are copied to the host. Returns name -> numpy row [min, max, n, sum, sumsq, zeros,
        counts...] (obs.summaries turns them into TensorBoard protos)."""
        from ..obs.events import BUCKET_EDGES
        if self.progSum is None:
            names, tensors = [], []
            for name, t in self.activations().items():
                if name != "G":
                    names.append(name + ("/activations" if name not in ("z", "d", "d_") else ""))
                    tensors.append(t)
            sharded = getattr(self, "_shards", None) is not None and self._sharded()
            for name, t in self.model.all_named_variables().items():
                if sharded and name.endswith("/w"):  # masters current only on this rank's shard:
                    mir = self.wbf_g if name in self.wbf_g.tensors else self.wbf_d  # the bf16 mirror
                    t = mir[name]
                names.append(name)
                tensors.append(t)
            nb = len(BUCKET_EDGES) + 1
            self._sum_edges = torch.tensor(BUCKET_EDGES, dtype=torch.float64, device=self.device)
            self._sum_out = torch.zeros(len(tensors), nb + 6, dtype=torch.float64, device=self.device)
            prog = self._prog()
            for i, t in enumerate(tensors):
                xd = 0 if t.dtype == torch.float32 else 1
                if xd == 1 and t.dtype != self.edt:
                    raise TypeError("summary of %s: dtype %s" % (names[i], t.dtype))
                prog.tensor_summary("sum." + names[i], _p(t), xd, t.numel(), _p(self._sum_edges), nb,
                                    _p(self._sum_out[i]), 0)
            self.progSum, self._sum_names = prog, names
        H.run(self.progSum)
        rows = self._sum_out.cpu().numpy()
        return OrderedDict(zip(self._sum_names, rows))

    # ------------------------------------------------------------------ sampling / eval
    def sampler(self, z: torch.Tensor, ema: Optional[bool] = None) -> torch.Tensor:
        """G with inference-mode BN (moving averages) -- distriubted_model.py:131-153. With
        --bn_zero_debias the moving averages are divided by 1 - decay^t (t = EMA updates so far,
        as in the reference engine's BNState.averages). ema: sample from the moving average of G's
        weights (``g_ema_decay`` > 0) instead of the last iterate; None = the average when kept."""
        use_ema = self.g_ema is not None if ema is None else bool(ema)
        if use_ema and self.g_ema is None:
            raise ValueError("sampler(ema=True) needs an engine built with g_ema_decay > 0")
        if use_ema:
            if self.progS_ema is None:
                self.progS_ema, self._s_out_ema = self._build_sampler(self.g_ema, self.wbf_g_ema)
            prog, out = self.progS_ema, self._s_out_ema
        else:
            if self.progS is None:
                self.progS, self._s_out = self._build_sampler(self.model.g, self.wbf_g)
            prog, out = self.progS, self._s_out
        bn = self.model.g_bn
        t = float(bn.steps[0])
        corr = 1.0 - bn.decay ** t if (bn.zero_debias and t > 0) else 1.0
        self._debias.fill_(1.0 / corr)
        self.sample_z.copy_(z.to(self.device, torch.float32))
        H.run(prog)
        return out.float().clone()

    def _build_sampler(self, Pg, Wg):
        """Sampler program over the fp32 parameter views Pg (projection, biases, BN scale / offset)
        and the conv kernels Wg the GEMMs read (16-bit mirror; fp32: Pg itself) -- G's weights, or
        their moving average. The BN moving averages and the debias scalar are shared."""
        cfg, B = self.cfg, self.B
        prog = self._prog()
        t = self._t
        h0p, h0 = t(B, cfg.g_lin_out), t(B, cfg.g_lin_out)
        s_out = t(B, cfg.output_size, cfg.output_size, cfg.c_dim)
        sc = {name: (t(C, dtype=torch.float32), t(C, dtype=torch.float32)) for name, C in cfg.g_bn_layers()}
        keep = [h0p, h0, sc]
        bnst = self.model.g_bn
        prog.linear_fwd("s.lin", _p(self.sample_z), _p(Pg["g_h0_lin/Matrix"]), _p(Pg["g_h0_lin/bias"]), _p(h0p), B,
                        cfg.z_dim, cfg.g_lin_out, 0)

        def coef(name, C):  # BN state and the debias factor are read live (device pointers)
            prog.bn_coef_eval("s." + name, C, _p(Pg[name + "/gamma"]), _p(Pg[name + "/beta"]), cfg.bn_eps,
                              _p(bnst.mean[name]), _p(bnst.var[name]), 1.0, _p(sc[name][0]), _p(sc[name][1]), 0,
                              _p(self._debias))

        C0 = cfg.g_base_ch
        coef("g_bn0", C0)
        prog.bn_apply_act("s.g_bn0", _p(h0p), _p(h0), _p(sc["g_bn0"][0]), _p(sc["g_bn0"][1]),
                          B * cfg.g_base_hw ** 2, C0, B * cfg.g_base_hw ** 2, RELU, 0.0, 0)
        prev = h0
        for L in self.gl:
            nat = Wg[L.name + "/w"]
            pad = same_pads(L.out_hw)[0]
            if L.bn:
                xb, ab = t(B, L.out_hw, L.out_hw, L.cout), t(B, L.out_hw, L.out_hw, L.cout)
                keep += [xb, ab]
                self._igemm(prog, "s." + L.name, H.GemmShape.fwd(L, B), prev, nat, xb, pad, bias=Pg[L.name + "/biases"])
                coef(L.bn, L.cout)
                rows = B * L.out_hw ** 2
                prog.bn_apply_act("s." + L.bn, _p(xb), _p(ab), _p(sc[L.bn][0]), _p(sc[L.bn][1]), rows, L.cout, rows,
                                  RELU, 0.0, 0)
                prev = ab
            else:
                self._deconv_out(prog, "s." + L.name, prev, nat, s_out, B, L, pad, Pg[L.name + "/biases"], TANH)
        self._s_keep = getattr(self, "_s_keep", []) + keep
        return prog, s_out

    def eval_losses(self, real: torch.Tensor, z: torch.Tensor) -> Dict[str, float]:
        """Sample-time d_loss / g_loss (image_train.py:181-184) in train-mode BN but WITHOUT
        mutating the moving averages (documented deviation)."""
        if self.progEval is None:
            prog = self._prog()
            self._ev_z = self._t(self.B, self.cfg.z_dim, dtype=torch.float32)
            self._build_forward(prog, update_ema=False, z=self._ev_z, train_z=False, noise=False)  # D sees clean inputs
            self.progEval = prog
        saved_real = self.d_in[:self.B].clone()
        saved_losses = self.losses.clone()
        self.set_batch(real, self.d_steps - 1)  # (the full step's slot: d_in)
        self._ev_z.copy_(z.to(self.device, torch.float32))
        H.run(self.progEval)
        l = self.losses.tolist()
        self.d_in[:self.B].copy_(saved_real)
        self.losses.copy_(saved_losses)
        return {"d_loss": l[3], "g_loss": l[2]}

    # ------------------------------------------------------------------ sliced Wasserstein distance
    def swd(self, real: Optional[torch.Tensor], z: torch.Tensor, patches: int, seed: int, ema: Optional[bool] = None,
            refresh: bool = False, max_rows: int = R.SWD_MAX_ROWS) -> List[float]:
        """Sliced Wasserstein distance x 1000 between `real` [n, S, S, C] and the n samples of z, per
        Laplacian-pyramid level, finest first (swd.hip; ops.hip.Swd). Programs of their own, recorded on
        first use: nothing of the training step is touched. The fakes come from ``sampler(z, ema=ema)`` in
        chunks of the batch size. The real side (its sorted projections per level) is computed on the first
        call and kept: later calls do not read `real` (None is fine) unless refresh is set or the set's
        size, `patches` or `seed` changed. max_rows: the largest n * patches accepted, a power of two in
        [32768, 2^21]; above 32768 the sorts are the global merge sort (ops.hip.Swd has the memory it takes)."""
        n, B = int(z.shape[0]), self.B
        R.check_swd(n, patches, self.cfg.output_size, max_rows=R.check_swd_max_rows(max_rows))
        key = (n, int(patches), int(seed))
        sw = getattr(self, "_swd", None)
        if sw is None or self._swd_key != key or refresh:
            if real is None or int(real.shape[0]) != n:
                raise ValueError("swd: the first evaluation needs the n = %d real images" % n)
            sw = H.Swd(n, self.cfg.output_size, self.cfg.c_dim, int(patches), int(seed), device=self.device)
            sw.set_real(real.to(self.device, torch.float32))
            self._swd, self._swd_key = sw, key
        z = z.to(self.device, torch.float32)
        for i in range(0, n, B):
            m = min(B, n - i)
            zc = z[i:i + m] if m == B else torch.cat([z[i:], z.new_zeros(B - m, z.shape[1])])
            sw.x[i:i + m].copy_(self.sampler(zc, ema=ema)[:m])
        return sw.distance()

    # ------------------------------------------------------------------ 1-NN two-sample test
    def nn_metric(self, real: Optional[torch.Tensor], z: torch.Tensor, size: Optional[int] = None,
                  ema: Optional[bool] = None, refresh: bool = False, k: int = 0, mmd: bool = False, fd: int = 0) -> dict:
        """The leave-one-out 1-NN two-sample test between `real` [n, S, S, C] and the n samples of z in the pixels
        of pyramid level `size` (None or 0: the images), and the nearest-real distances (nn.hip; ops.hip.NnMetric):
        {"acc", "acc_real", "acc_fake", "dist_fr", "dist_rr", "nearest"}, `nearest` the index of every fake's
        nearest real image. Programs of their own, recorded on first use: nothing of the training step is
        touched. The fakes come from ``sampler(z, ema=ema)`` in chunks of the batch size. The real side (features,
        mean and its own leave-one-out search) is computed on the first call and kept: later calls do not read
        `real` (None is fine) unless refresh is set or the set's size, `size`, k, mmd or fd changed. k > 0 adds the k-NN
        manifold estimates "precision", "recall", "density", "coverage" and "k" (ops.hip.NnMetric.prdc); mmd adds the
        kernel MMD's "mmd2", "k_rr", "k_ff", "k_rf" and "h" (ops.hip.NnMetric.mmd); fd > 0 adds the Frechet distance's
        "fd", "fd_mean2", "fd_tr", "fd_nuc" and "fd_tail" from fd steps of the polar iteration (ops.hip.NnMetric.frechet)."""
        n, B = int(z.shape[0]), self.B
        key = (n, R.check_nn(n, size, self.cfg.output_size), R.check_nn_k(k, n, least=0), R.check_nn_mmd(mmd, n),
               R.check_nn_fd(fd, n))
        nn = getattr(self, "_nn", None)
        if nn is None or self._nn_key != key or refresh:
            if real is None or int(real.shape[0]) != n:
                raise ValueError("nn_metric: the first evaluation needs the n = %d real images" % n)
            nn = H.NnMetric(n, self.cfg.output_size, self.cfg.c_dim, key[1], device=self.device, k=key[2], mmd=key[3],
                            fd=key[4])
            nn.set_real(real.to(self.device, torch.float32))
            self._nn, self._nn_key = nn, key
        z = z.to(self.device, torch.float32)
        for i in range(0, n, B):
            m = min(B, n - i)
            zc = z[i:i + m] if m == B else torch.cat([z[i:], z.new_zeros(B - m, z.shape[1])])
            nn.x[i:i + m].copy_(self.sampler(zc, ema=ema)[:m])
        out = R.nn_report(nn())
        if key[2]:
            out.update(R.nn_prdc_report(nn.prdc()))
        if key[3]:
            out.update(R.nn_mmd_report(nn.mmd()))
        if key[4]:
            out.update(R.nn_fd_report(nn.frechet()))
        return out

    def placement(self) -> List[str]:
        """--log_device_placement lines: every recorded op of the step runs on this rank's HIP
        device; which stream slots / graphs carry it."""
        progs = [("forward+G backward", self.progA), ("D backward", self.progB), ("G weight grads", self.progW),
                 ("optimisers", self.progC)]
        for k, (pf, pb) in enumerate(self._sub):
            progs += [("D sub-step %d forward" % k, pf), ("D sub-step %d D backward" % k, pb)]
        if self._sub:
            progs.append(("D sub-step update", self.progDU))
        out = ["HIP engine (%s): %d kernels per step, schedule %s, hipGraph %s%s" % (
            self.dtype_name, self.kernel_count(), self._schedule(), "captured" if self.graph_enabled else
            ("requested" if self.graph_requested else "off"),
            ", comm stream for all-reduces" if self.ddp else "")]
        for label, p in progs:
            if p is None:
                continue
            slots = sorted({p.op_info(i)[1] for i in range(p.size())})
            out.append("  %-20s %3d ops on %s, stream slots %s" % (label, p.size(), self.device, slots))
        return out

    def _step_progs(self):
        subs = [p for pair in self._sub for p in pair] + [self.progDU] * len(self._sub)
        ada = getattr(self, "progAda", None)  # (listed where the schedule issues it on the D chain's stream)
        chain = (self.progB, ada) if self._schedule() == "fused" and self._ada_at_tail() else (ada, self.progB)
        return [p for p in (self.progA,) + chain + (self.progW, self.progC, getattr(self, "progSh", None))
                if p is not None] + subs

    def sub_op_names(self, k: int) -> List[str]:
        """Names of the recorded ops of D sub-step k: forward, D chain, update."""
        out = []
        for p in self._sub[k] + (self.progDU,):
            out += [p.name(i) for i in range(p.size())]
        return out

    def op_names(self) -> List[str]:
        out = []
        for p in self._step_progs():
            out += [p.name(i) for i in range(p.size())]
        return out

    def kernel_count(self) -> int:
        """Kernel launches per training step (events excluded)."""
        n = 0
        for p in self._step_progs():
            n += sum(1 for i in range(p.size()) if p.op_info(i)[2] == self.ext.OP_LAUNCH)
        return n
