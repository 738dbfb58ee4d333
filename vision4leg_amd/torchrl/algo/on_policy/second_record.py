"""The shell of the learners whose update writes a second statistics record next to PPO's (VMPO, A2C, Reinforce): what they
refuse, and a run of U updates on the trainer's stream whose two record arrays come back in one device-to-host copy. All updates of an epoch
are ONE hipGraph replay, like PPO's (V4L_EPOCH_GRAPH=0: one replay per update; V4L_GRAPH=0: eager launches; update(batch): the
single-update replay). Construction, the collector / buffer wiring, train(), snapshot and process_epoch_samples are PPO's.

A subclass declares:
  _second_stats   floats per update of its record
  _rollout_keys   the host batch's keys it hands to HipTrainer.rollout, a prefix of PPO's (acts, advs, estimate_returns, values)
  _passes         passes over the samples per epoch
  _syncs_target   trainer.sync_target() at the start of an epoch
  _run_entry, _next_entry   the HipTrainer methods that run U updates / the next update
  _info(row, second_row)    the logger's info dict of one update from the two records
and may override _lr_vf() (the critic's learning rate handed to the opening launch: Reinforce keeps no public vf_optimizer).
"""
import os

import torch

from . import ppo as _ppo
from .ppo import PPO, _check_update_records
from ... import replay_buffers as rb
from .... import _lib
from ....engine import HipTrainer


class _SecondRecordPPO(PPO):
    def _refuse(self, pf, kwargs):
        """What neither learner takes; called before PPO.__init__, so before anything touches a device."""
        name = type(self).__name__
        if getattr(pf, "logstd_head", False):
            raise NotImplementedError("vision4leg_amd: %s does not take policies.GaussianContPolicy (log-std from the head): its "
                                      "loss kernel takes one log-std per action column; the policy runs under algo.PPO" % name)
        if kwargs.get("skip_nonfinite_steps"):
            raise NotImplementedError("vision4leg_amd: %s does not take skip_nonfinite_steps=True (the guard covers PPO's update "
                                      "and its two optimisers only)" % name)
        if kwargs.get("target_kl") is not None:
            raise NotImplementedError("vision4leg_amd: %s does not take target_kl (the KL early stop belongs to PPO's update: "
                                      "its passes over the same samples, its ratio's log pi_old)" % name)
        if kwargs.get("desired_kl") is not None:
            raise NotImplementedError("vision4leg_amd: %s does not take desired_kl (the KL-adaptive learning rates belong to PPO's "
                                      "update: its passes over the same samples, its ratio's log pi_old)" % name)
        if kwargs.get("save_train_state") or kwargs.get("resume") is not None:
            raise NotImplementedError("vision4leg_amd: %s does not save or resume a train state (what its update adds is not part "
                                      "of it); snapshot() writes the reference's model files" % name)
        forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                  and torch.distributed.is_initialized())
        if _ppo._dist_world() > 1 or forced:
            raise NotImplementedError("vision4leg_amd: %s runs in a single process (no data-parallel %s update: "
                                      "world_size > 1 / V4L_FORCE_DP_PHASES)" % (name, name))

    def train_state(self):
        raise NotImplementedError("vision4leg_amd: %s has no resumable train state" % type(self).__name__)

    def save_checkpoint(self, prefix, epoch):
        raise NotImplementedError("vision4leg_amd: %s has no resumable train state; use snapshot()" % type(self).__name__)

    def load_checkpoint(self, prefix, epoch, restore_rng=True, restore_collector=False):
        raise NotImplementedError("vision4leg_amd: %s has no resumable train state" % type(self).__name__)

    def run_updates(self, ro, rowidx, stats, skip=None):
        raise NotImplementedError("vision4leg_amd: %s's updates are run by update() / update_per_epoch()" % type(self).__name__)

    # ---- epoch (v_mpo.py:44-56, on_rl_algo.py:36-41: no learning-rate schedule)
    def update_per_epoch(self):
        with torch.cuda.device(self.device):
            self.process_epoch_samples()
            if self._syncs_target:
                self.trainer.sync_target()  # copy_model_params_from_to(pf, target_pf), v_mpo.py:50
            if isinstance(self.replay_buffer, rb.DeviceOnPolicyReplayBuffer):
                self._update_epoch_resident()
                return
            for _ in range(self._passes):
                for batch in self.replay_buffer.one_iteration(self.batch_size, self.sample_key, self.shuffle):
                    infos = self.update(batch)
                    self.logger.add_update_info(infos)

    def _buffers(self, rowidx, U):
        """The row-index tensor and both record arrays of a run of U updates — one allocation: [U][V4L_STATS] PPO records, then
        [U][_second_stats] — at one address from run to run (the captured graphs are keyed on them): reallocated only when the
        shape changes."""
        shape = (U, None if rowidx is None else tuple(rowidx.shape))
        if getattr(self, "_buf_shape", None) != shape:
            self._buf_shape = shape
            self._rows_buf = None if rowidx is None else torch.empty_like(rowidx)
            self._both_buf = torch.zeros(U * (_lib.V4L_STATS + self._second_stats), dtype=torch.float32, device=self.device)
            self._first_buf = self._both_buf[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS)
            self._second_buf = self._both_buf[U * _lib.V4L_STATS:].view(U, self._second_stats)
        if rowidx is not None:
            self._rows_buf.copy_(rowidx)
        return self._rows_buf, self._both_buf, self._first_buf, self._second_buf

    def _lr_vf(self):
        """The critic's learning rate of the run being opened (a learner that keeps no public vf_optimizer overrides this)."""
        return self.vf_optimizer.lr

    def _run(self, ro, rowidx, n, U, what):
        """U updates on rows rowidx[u] (None: rows 0 .. n-1) on the trainer's stream, then ONE device-to-host copy of both record
        arrays and the host's checks. -> list of U info dicts. The whole run is ONE hipGraph replay (one replay per update with
        V4L_EPOCH_GRAPH=0, eager launches with V4L_GRAPH=0), by PPO.run_updates' switches."""
        tr = self.trainer
        rows, rec, stats, second = self._buffers(rowidx, U)
        cur = torch.cuda.current_stream(self.device)
        tr.stream.wait_stream(cur)
        with torch.cuda.stream(tr.stream):
            tr._pre(n)
            tr.begin(rows, stats, self.pf_optimizer.lr, self._lr_vf())
            self.training_update_num += U
            if self.use_graph and os.environ.get("V4L_EPOCH_GRAPH", "1") != "0":
                getattr(tr, self._run_entry)(ro, n, U, second, graph=True)
            else:
                for _ in range(U):
                    getattr(tr, self._next_entry)(ro, n, second, graph=self.use_graph)
            host = rec.cpu().numpy()  # the only device->host sync of the run
        cur.wait_stream(tr.stream)
        hs = host[:U * _lib.V4L_STATS].reshape(U, _lib.V4L_STATS)
        h2 = host[U * _lib.V4L_STATS:].reshape(U, self._second_stats)
        _check_update_records(hs, None, False, what)
        self._note_f16_saturation(float(hs[:, _lib.ST_F16_SAT].sum()))
        return [self._info(hs[u], h2[u]) for u in range(U)]

    def _update_epoch_resident(self):
        # device_rollout(): state, image, then acts, advs, rets, vals, log pi_old — the order of PPO's keys; no learner here
        # reads a stored log pi_old
        state, image, *arrays = self.replay_buffer.device_rollout()
        ro = HipTrainer.rollout(state, image, *arrays[:len(self._rollout_keys)])
        rowidx = self._epoch_rowidx(self._passes)
        U, n = rowidx.shape
        for info in self._run(ro, rowidx, n, U, lambda u: "minibatch update %d of epoch %d" % (u, self.current_epoch)):
            self.logger.add_update_info(info)

    def update(self, batch):
        """One minibatch update from a reference-style host batch (v_mpo.py:157-184, a2c.py:46-107). Returns _info's dict."""
        with torch.cuda.device(self.device):
            n, new = self._upload_batch(batch, self._rollout_keys)
            # the rollout arrays keep their addresses from call to call (the single-update graph is keyed on them)
            held = getattr(self, "_held", None)
            if held is None or any(h.shape != v.shape for h, v in zip(held, new)):
                held = self._held = [torch.empty_like(v) for v in new]
            for h, v in zip(held, new):
                h.copy_(v)
            ro = HipTrainer.rollout(self._stage[0], self._stage[1], *held)
            return self._run(ro, None, n, 1, lambda u: "minibatch update %d" % self.training_update_num)[0]
