"""A2C with the reference's constructor, attributes and epoch protocol (torchrl/algo/on_policy/a2c.py:8-114 on top of
on_rl_algo.py:11-48, rl_algo.py:19-168), on the PPO shell of this package: construction, the collector / buffer wiring, train(),
snapshot and process_epoch_samples are PPO's.

What differs is the update (a2c.py:46-107): no ratio, no target policy, an MSE critic and ONE pass over the epoch's samples
(on_rl_algo.py:36-41), with no learning-rate schedule. Two single-block launches of its own (a2c_critic_loss_kernel,
a2c_loss_kernel) sit between PPO's opening launch, forwards, backwards and clip + Adam launches (max_grad_norm 0.5, a2c.py:81,86).
All updates of an epoch are ONE hipGraph replay on the trainer's stream, like PPO's (V4L_EPOCH_GRAPH=0: one replay per update;
V4L_GRAPH=0: eager launches; update(batch): the single-update replay); with a DeviceOnPolicyReplayBuffer the records of all
updates of an epoch come back in one device-to-host copy.

State-MLP nets (networks.Net pairs, the `ppo_state.py` workload) only. The reference's A2C evaluates vf(obs) before
pf_optimizer.step() and backpropagates vf_loss after it (a2c.py:76-85): with a parameter common to pf and vf torch raises
"one of the variables needed for gradient computation has been modified by an inplace operation", and every vision starter hands
one encoder object to both nets — so the reference's A2C runs networks.Net pairs and nothing else the starters build. With
disjoint parameter sets the two optimiser steps are independent and the update keeps the PPO update's critic-first launch order.

Not supported, refused at construction: any other net kind, pf and vf with a common parameter, data parallel (world_size > 1,
V4L_FORCE_DP_PHASES), skip_nonfinite_steps, save_train_state / resume.
"""
import os

import numpy as np
import torch
import torch.optim as optim

from . import ppo as _ppo
from .ppo import PPO, _check_update_records
from ... import replay_buffers as rb
from .... import _lib
from ....engine import HipTrainer


def _is_state_mlp(net):
    cfg = getattr(net, "_net_cfg", None)
    return cfg is not None and cfg().kind == _lib.V4L_NET_MLP  # (host only: no engine handle is made)


class A2C(PPO):
    def __init__(self, pf, vf, plr=3e-4, vlr=3e-4, optimizer_class=optim.Adam, entropy_coeff=0.001, shuffle=True, tau=None, gae=True,
                 **kwargs):
        if getattr(pf, "logstd_head", False):
            raise NotImplementedError("vision4leg_amd: A2C does not take policies.GaussianContPolicy (log-std from the head): the "
                                      "A2C loss kernel takes one log-std per action column; the policy runs under algo.PPO")
        if not (_is_state_mlp(pf) and _is_state_mlp(vf)):
            raise NotImplementedError("vision4leg_amd: A2C runs state-MLP nets (networks.Net pairs) only: the reference's A2C "
                                      "raises on a shared encoder (vf(obs) is evaluated before pf_optimizer.step() and "
                                      "backpropagated after it, a2c.py:76-85), and every vision starter shares one")
        if {id(p) for p in pf.parameters()} & {id(p) for p in vf.parameters()}:
            raise NotImplementedError("vision4leg_amd: A2C needs pf and vf without a common parameter: the reference's A2C raises "
                                      "on shared parameters (an in-place optimiser step between vf(obs) and vf_loss.backward())")
        if kwargs.get("skip_nonfinite_steps"):
            raise NotImplementedError("vision4leg_amd: A2C does not take skip_nonfinite_steps=True (the guard is not part of the "
                                      "A2C update)")
        if kwargs.get("save_train_state") or kwargs.get("resume") is not None:
            raise NotImplementedError("vision4leg_amd: A2C does not save or resume a train state; snapshot() writes the reference's "
                                      "model files")
        forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                  and torch.distributed.is_initialized())
        if _ppo._dist_world() > 1 or forced:
            raise NotImplementedError("vision4leg_amd: A2C runs in a single process (no data-parallel A2C update: "
                                      "world_size > 1 / V4L_FORCE_DP_PHASES)")
        for k in ("clip_para", "opt_epochs", "clipped_value_loss"):  # PPO's, not A2C's (a2c.py:13-20)
            if k in kwargs:
                raise TypeError("A2C.__init__() got an unexpected keyword argument %r" % k)
        # clip_para is never read by an A2C launch; one pass over the samples (on_rl_algo.py:36-41)
        super().__init__(pf, vf, plr=plr, vlr=vlr, optimizer_class=optimizer_class, entropy_coeff=entropy_coeff, clip_para=0.0,
                         opt_epochs=1, clipped_value_loss=False, shuffle=shuffle, tau=tau, gae=gae, **kwargs)
        # the trainer's third net handle is never run by an A2C update: kept private, no `target_pf` on the surface
        self._target_pf = self.__dict__.pop("target_pf")
        for k in ("clip_para", "opt_epochs", "clipped_value_loss"):
            self.__dict__.pop(k)
        self.sample_key = ["obs", "acts", "advs", "estimate_returns"]  # on_rl_algo.py:18

    @property
    def networks(self):
        return [self.pf, self.vf]  # on_rl_algo.py:43-48

    def to(self, device):
        hidden = self.__dict__.get("target_pf", self.__dict__.get("_target_pf"))
        for net in self.networks + ([hidden] if hidden is not None else []):
            net.to(device)

    # ---- not part of A2C here
    def train_state(self):
        raise NotImplementedError("vision4leg_amd: A2C has no resumable train state")

    def save_checkpoint(self, prefix, epoch):
        raise NotImplementedError("vision4leg_amd: A2C has no resumable train state; use snapshot()")

    def load_checkpoint(self, prefix, epoch, restore_rng=True, restore_collector=False):
        raise NotImplementedError("vision4leg_amd: A2C has no resumable train state")

    # ---- epoch (on_rl_algo.py:36-41: one pass, no learning-rate schedule, no target sync)
    def update_per_epoch(self):
        with torch.cuda.device(self.device):
            self.process_epoch_samples()
            if isinstance(self.replay_buffer, rb.DeviceOnPolicyReplayBuffer):
                self._update_epoch_resident()
                return
            for batch in self.replay_buffer.one_iteration(self.batch_size, self.sample_key, self.shuffle):
                infos = self.update(batch)
                self.logger.add_update_info(infos)

    def _buffers(self, rowidx, U):
        """The row-index tensor and both record arrays of a run of U updates — one allocation: [U][V4L_STATS] PPO records, then
        [U][V4L_A2C_STATS] — at one address from run to run (the captured graphs are keyed on them): reallocated only when the
        shape changes."""
        shape = (U, None if rowidx is None else tuple(rowidx.shape))
        if getattr(self, "_abuf_shape", None) != shape:
            self._abuf_shape = shape
            self._arowidx_buf = None if rowidx is None else torch.empty_like(rowidx)
            self._arec_buf = torch.zeros(U * (_lib.V4L_STATS + _lib.V4L_A2C_STATS), dtype=torch.float32, device=self.device)
            self._apstats_buf = self._arec_buf[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS)
            self._astats_buf = self._arec_buf[U * _lib.V4L_STATS:].view(U, _lib.V4L_A2C_STATS)
        if rowidx is not None:
            self._arowidx_buf.copy_(rowidx)
        return self._arowidx_buf, self._arec_buf, self._apstats_buf, self._astats_buf

    def _run(self, ro, rowidx, n, U, what):
        """U updates on rows rowidx[u] (None: rows 0 .. n-1) on the trainer's stream, then ONE device-to-host copy of both record
        arrays and the host's checks. -> list of U info dicts. The whole run is ONE hipGraph replay (one replay per update with
        V4L_EPOCH_GRAPH=0, eager launches with V4L_GRAPH=0), by PPO.run_updates' switches."""
        tr = self.trainer
        rows, rec, stats, astats = self._buffers(rowidx, U)
        cur = torch.cuda.current_stream(self.device)
        tr.stream.wait_stream(cur)
        with torch.cuda.stream(tr.stream):
            tr._pre(n)
            tr.begin(rows, stats, self.pf_optimizer.lr, self.vf_optimizer.lr)
            self.training_update_num += U
            if self.use_graph and os.environ.get("V4L_EPOCH_GRAPH", "1") != "0":
                tr.a2c_update_run(ro, n, U, astats, graph=True)
            else:
                for _ in range(U):
                    tr.a2c_update_next(ro, n, astats, graph=self.use_graph)
            host = rec.cpu().numpy()  # the only device->host sync of the run
        cur.wait_stream(tr.stream)
        hs = host[:U * _lib.V4L_STATS].reshape(U, _lib.V4L_STATS)
        ha = host[U * _lib.V4L_STATS:].reshape(U, _lib.V4L_A2C_STATS)
        _check_update_records(hs, None, False, what)
        self._note_f16_saturation(float(hs[:, _lib.ST_F16_SAT].sum()))
        return [self._info(ha[u], None) for u in range(U)]

    def _update_epoch_resident(self):
        buf = self.replay_buffer
        state, image, acts, advs, rets, _, _ = buf.device_rollout()
        ro = HipTrainer.rollout(state, image, acts, advs, rets)  # (no stored values, no stored log pi_old: A2C reads neither)
        batches = [b["rowidx"] for b in buf.one_iteration(self.batch_size, self.sample_key, self.shuffle)]
        rowidx = torch.from_numpy(np.stack(batches)).to(self.device)  # one upload per epoch
        U, n = rowidx.shape
        for info in self._run(ro, rowidx, n, U, lambda u: "minibatch update %d of epoch %d" % (u, self.current_epoch)):
            self.logger.add_update_info(info)

    def _info(self, row, flags):
        """The logger's info dict of one update: the reference's 12 keys in its order (a2c.py:89-105)."""
        return {k: float(row[j]) for j, k in enumerate(_lib.A2C_INFO_KEYS)}

    def run_updates(self, ro, rowidx, stats, skip=None):
        raise NotImplementedError("vision4leg_amd: A2C's updates are run by update() / update_per_epoch()")

    def update(self, batch):
        """One minibatch update from a reference-style host batch (a2c.py:46-107; no "values" key). Returns the 12-key info."""
        if "rowidx" in batch:
            raise RuntimeError("device-resident batches are consumed by update_per_epoch")
        dev = self.device
        with torch.cuda.device(dev):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
            obs = up(batch["obs"])
            n = obs.shape[0]
            net = self.pf.hip
            net.ensure_bound()
            if self._stage is None or self._stage[0].shape[0] != n:
                self._stage = net.alloc_rollout(n, dev)
            net.ingest(obs, self._stage[0], self._stage[1])
            # the rollout arrays keep their addresses from call to call (the single-update graph is keyed on them)
            new = {"acts": up(batch["acts"]).reshape(n, -1), "advs": up(batch["advs"]).reshape(n),
                   "rets": up(batch["estimate_returns"]).reshape(n)}
            held = getattr(self, "_astage", None)
            if held is None or any(held[k].shape != v.shape for k, v in new.items()):
                held = self._astage = {k: torch.empty_like(v) for k, v in new.items()}
            for k, v in new.items():
                held[k].copy_(v)
            ro = HipTrainer.rollout(self._stage[0], self._stage[1], held["acts"], held["advs"], held["rets"])
            return self._run(ro, None, n, 1, lambda u: "minibatch update %d" % self.training_update_num)[0]
