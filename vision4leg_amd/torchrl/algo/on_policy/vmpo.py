"""V-MPO with the reference's constructor, attributes and epoch protocol (torchrl/algo/on_policy/v_mpo.py:11-192 on top of
a2c.py:13-44, on_rl_algo.py:11-34, rl_algo.py:19-168), on the PPO shell of this package: construction, the collector / buffer
wiring, train(), snapshot and process_epoch_samples are PPO's.

What differs is the actor stage of a minibatch update (v_mpo.py:58-134): the better half of the minibatch by normalised
advantage is chosen on the device (vmpo_select_kernel), the live and the frozen target policy run on those rows, and one
single-block launch (vmpo_loss_kernel) forms the softmax-weighted log-prob + alpha KL loss, its gradients, the statistics and
the Adam step of the two learnable scalars eta and alpha. The critic step, the clip + Adam launches and the advantage statistics
are PPO's with clipped_value_loss=False. All updates of an epoch are ONE hipGraph replay on the trainer's stream, like PPO's
(V4L_EPOCH_GRAPH=0: one replay per update; V4L_GRAPH=0: eager launches; update(batch): the single-update replay); with a
DeviceOnPolicyReplayBuffer the records of all updates of an epoch come back in one device-to-host copy.

Not supported, refused at construction: data parallel (world_size > 1, V4L_FORCE_DP_PHASES), skip_nonfinite_steps,
save_train_state / resume (the reference's snapshot holds neither eta nor alpha; snapshot() keeps writing the reference's files).
"""
import os

import numpy as np
import torch

from . import ppo as _ppo
from .ppo import PPO, _check_update_records
from ... import replay_buffers as rb
from .... import _lib
from ....engine import HipTrainer


class _ScalarAdam:
    """`param_optimizer` of the reference (v_mpo.py:35-39): `optimizer_class([eta, alpha], lr=plr, eps=1e-5)`. Its state lives in
    the trainer's V-MPO device block and its step is taken inside the loss launch, at the policy optimiser's learning rate (the
    reference runs both at plr: V-MPO has no schedule). This object reports the group's values."""

    def __init__(self, plr, eps, betas, weight_decay, decoupled):
        self.param_groups = [{"params": ["eta", "alpha"], "lr": plr, "eps": eps, "betas": betas, "weight_decay": weight_decay,
                              "decoupled_weight_decay": bool(decoupled)}]

    def zero_grad(self):
        pass


class VMPO(PPO):
    def __init__(self, pf, vf, opt_epochs=10, eta_eps=0.02, alpha_eps=0.1, clipped_value_loss=False, **kwargs):
        if getattr(pf, "logstd_head", False):
            raise NotImplementedError("vision4leg_amd: VMPO does not take policies.GaussianContPolicy (log-std from the head): the "
                                      "V-MPO loss kernel takes one log-std per action column; the policy runs under algo.PPO")
        if kwargs.get("skip_nonfinite_steps"):
            raise NotImplementedError("vision4leg_amd: VMPO does not take skip_nonfinite_steps=True (the guard covers PPO's two "
                                      "optimisers, not eta / alpha)")
        if kwargs.get("save_train_state") or kwargs.get("resume") is not None:
            raise NotImplementedError("vision4leg_amd: VMPO does not save or resume a train state (eta, alpha and their optimiser "
                                      "are not part of it); snapshot() writes the reference's model files")
        forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                  and torch.distributed.is_initialized())
        if _ppo._dist_world() > 1 or forced:
            raise NotImplementedError("vision4leg_amd: VMPO runs in a single process (no data-parallel V-MPO update: "
                                      "world_size > 1 / V4L_FORCE_DP_PHASES)")
        # the critic step is plain MSE whatever clipped_value_loss says (v_mpo.py:136-155): stored, ignored, as in the reference
        super().__init__(pf, vf, opt_epochs=opt_epochs, clipped_value_loss=False, **kwargs)
        self.clipped_value_loss = clipped_value_loss
        self.eta_eps, self.alpha_eps = eta_eps, alpha_eps
        g = self.pf_optimizer.param_groups[0]
        self.param_optimizer = _ScalarAdam(self.plr, g["eps"], g["betas"], g["weight_decay"], g["decoupled_weight_decay"])
        with torch.cuda.device(self.device):
            self.trainer.vmpo_init(eta_eps, alpha_eps, eta0=1.0, alpha0=0.1)  # v_mpo.py:28,32

    # ---- the two learnable scalars, read from the device (one synchronise each)
    def _scalar(self, i):
        with torch.cuda.device(self.device):
            return torch.tensor([self.trainer.vmpo_state()[i]], dtype=torch.float32, device=self.device)

    @property
    def eta(self):
        return self._scalar(0)

    @property
    def alpha(self):
        return self._scalar(1)

    # ---- not part of V-MPO here
    def train_state(self):
        raise NotImplementedError("vision4leg_amd: VMPO has no resumable train state")

    def save_checkpoint(self, prefix, epoch):
        raise NotImplementedError("vision4leg_amd: VMPO has no resumable train state; use snapshot()")

    def load_checkpoint(self, prefix, epoch, restore_rng=True, restore_collector=False):
        raise NotImplementedError("vision4leg_amd: VMPO has no resumable train state")

    # ---- epoch (v_mpo.py:44-56: no learning-rate schedule)
    def update_per_epoch(self):
        with torch.cuda.device(self.device):
            self.process_epoch_samples()
            self.trainer.sync_target()  # copy_model_params_from_to(pf, target_pf), v_mpo.py:50
            if isinstance(self.replay_buffer, rb.DeviceOnPolicyReplayBuffer):
                self._update_epoch_resident()
                return
            for _ in range(self.opt_epochs):
                for batch in self.replay_buffer.one_iteration(self.batch_size, self.sample_key, self.shuffle):
                    infos = self.update(batch)
                    self.logger.add_update_info(infos)

    def _buffers(self, rowidx, U):
        """The row-index tensor and both record arrays of a run of U updates — one allocation: [U][V4L_STATS] PPO records, then
        [U][V4L_VMPO_STATS] — at one address from run to run (the captured graphs are keyed on them): reallocated only when the
        shape changes."""
        shape = (U, None if rowidx is None else tuple(rowidx.shape))
        if getattr(self, "_vbuf_shape", None) != shape:
            self._vbuf_shape = shape
            self._vrowidx_buf = None if rowidx is None else torch.empty_like(rowidx)
            self._vrec_buf = torch.zeros(U * (_lib.V4L_STATS + _lib.V4L_VMPO_STATS), dtype=torch.float32, device=self.device)
            self._vpstats_buf = self._vrec_buf[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS)
            self._vstats_buf = self._vrec_buf[U * _lib.V4L_STATS:].view(U, _lib.V4L_VMPO_STATS)
        if rowidx is not None:
            self._vrowidx_buf.copy_(rowidx)
        return self._vrowidx_buf, self._vrec_buf, self._vpstats_buf, self._vstats_buf

    def _run(self, ro, rowidx, n, U, what):
        """U updates on rows rowidx[u] (None: rows 0 .. n-1) on the trainer's stream, then ONE device-to-host copy of both record
        arrays and the host's checks. -> list of U info dicts. The whole run is ONE hipGraph replay (one replay per update with
        V4L_EPOCH_GRAPH=0, eager launches with V4L_GRAPH=0), by PPO.run_updates' switches."""
        tr = self.trainer
        rows, rec, stats, vstats = self._buffers(rowidx, U)
        cur = torch.cuda.current_stream(self.device)
        tr.stream.wait_stream(cur)
        with torch.cuda.stream(tr.stream):
            tr._pre(n)
            tr.begin(rows, stats, self.pf_optimizer.lr, self.vf_optimizer.lr)
            self.training_update_num += U
            if self.use_graph and os.environ.get("V4L_EPOCH_GRAPH", "1") != "0":
                tr.vmpo_update_run(ro, n, U, vstats, graph=True)
            else:
                for _ in range(U):
                    tr.vmpo_update_next(ro, n, vstats, graph=self.use_graph)
            host = rec.cpu().numpy()  # the only device->host sync of the run
        cur.wait_stream(tr.stream)
        hs = host[:U * _lib.V4L_STATS].reshape(U, _lib.V4L_STATS)
        hv = host[U * _lib.V4L_STATS:].reshape(U, _lib.V4L_VMPO_STATS)
        _check_update_records(hs, None, False, what)
        self._note_f16_saturation(float(hs[:, _lib.ST_F16_SAT].sum()))
        return [self._info(hs[u], hv[u]) for u in range(U)]

    def _update_epoch_resident(self):
        buf = self.replay_buffer
        state, image, acts, advs, rets, vals, _ = buf.device_rollout()
        ro = HipTrainer.rollout(state, image, acts, advs, rets, vals)  # (no stored log pi_old: the KL needs the target's mean)
        batches = []
        for _ in range(self.opt_epochs):
            for b in buf.one_iteration(self.batch_size, self.sample_key, self.shuffle):
                batches.append(b["rowidx"])
        rowidx = torch.from_numpy(np.stack(batches)).to(self.device)  # one upload per epoch
        U, n = rowidx.shape
        for info in self._run(ro, rowidx, n, U, lambda u: "minibatch update %d of epoch %d" % (u, self.current_epoch)):
            self.logger.add_update_info(info)

    def _info(self, row, vrow):
        """The logger's info dict of one update: the reference's 19 keys (v_mpo.py:119-134, 154-155, 173-176)."""
        both = {k: float(row[j]) for j, k in enumerate(_lib.STAT_KEYS)}
        both.update({k: float(vrow[j]) for j, k in enumerate(_lib.VMPO_STAT_KEYS)})
        return {k: both[k] for k in _lib.VMPO_INFO_KEYS}

    def run_updates(self, ro, rowidx, stats, skip=None):
        raise NotImplementedError("vision4leg_amd: VMPO's updates are run by update() / update_per_epoch()")

    def update(self, batch):
        """One minibatch update from a reference-style host batch (v_mpo.py:157-184). Returns the 19-key info."""
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
                   "rets": up(batch["estimate_returns"]).reshape(n), "vals": up(batch["values"]).reshape(n)}
            held = getattr(self, "_vstage", None)
            if held is None or any(held[k].shape != v.shape for k, v in new.items()):
                held = self._vstage = {k: torch.empty_like(v) for k, v in new.items()}
            for k, v in new.items():
                held[k].copy_(v)
            ro = HipTrainer.rollout(self._stage[0], self._stage[1], held["acts"], held["advs"], held["rets"], held["vals"])
            return self._run(ro, None, n, 1, lambda u: "minibatch update %d" % self.training_update_num)[0]
