"""PPO with the reference's constructor, attributes and epoch protocol
(torchrl/algo/on_policy/ppo.py:10-161 on top of a2c.py:13-44, on_rl_algo.py:11-34, rl_algo.py:19-168).

What changes is *where* the work runs: `update` enqueues one fused critic-then-actor minibatch update on the
MI355X (forward, loss, backward, global-norm clip and Adam for both optimisers, all hand-written HIP behind
libv4l_hip.so) and `process_epoch_samples` runs the last-value forward and the fp64 GAE kernel. With a
`DeviceOnPolicyReplayBuffer` the observations never leave HBM and the 18 logger scalars of all 48 updates are
read back once per epoch instead of 18 `.item()` syncs per update.

Data parallel (one process per GPU, torch.distributed "nccl" == RCCL): every rank owns an env shard and its own
rollout; gradients are summed with ONE all-reduce per optimiser step on the flat gradient buffer (the critic's
carries the 3 advantage-normalisation scalars in its tail), then clipped and applied identically on every rank.
"""
import copy
import os
import os.path as osp
import pathlib
import pickle
import time
from collections import deque

import numpy as np
import torch

from .. import utils as atu
from ... import replay_buffers as rb
from .... import _lib
from .... import optim as hip_optim
from .... import train_state as ts
from ....engine import HipTrainer


class _HipAdam:
    """Optimiser facade: the Adam state lives in the trainer's flat device buffers; this object carries the learning rate so
    `update_linear_schedule` and user code can read/write `param_groups[0]['lr']`, and — once PPO has attached the trainer —
    reads and writes that state in `torch.optim.Adam`'s own `state_dict()` format (vision4leg_amd/train_state.py). The other
    group values (betas, eps, weight_decay, decoupled_weight_decay) are what PPO resolved from `optimizer_class` and handed to the
    trainer: they are fixed, and a state written under other values does not load."""

    def __init__(self, params, lr, eps=1e-5, betas=(0.9, 0.999), weight_decay=0, decoupled_weight_decay=False):
        self.param_groups = [{"params": list(params), "lr": lr, "eps": eps, "betas": betas, "weight_decay": weight_decay,
                              "decoupled_weight_decay": bool(decoupled_weight_decay)}]
        self._trainer = None

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def zero_grad(self):
        pass

    def attach(self, trainer, side, module):
        """side: 0 = the trainer's pf buffers and count, 1 = vf's; module: the net whose parameters() this optimiser owns."""
        self._trainer, self._side, self._module = trainer, side, module

    def _slices(self):
        if self._trainer is None:
            raise RuntimeError("vision4leg_amd: this optimiser facade is not attached to a trainer (PPO.__init__ does that)")
        net = self._trainer.vf if self._side else self._trainer.pf
        return net, ts.param_slices(net, self._module)

    def state_dict(self):
        """What `optimizer_class(net.parameters(), lr=..., eps=1e-5).state_dict()` would hold after the same steps."""
        _, slices = self._slices()
        state = self._trainer.adam_state()
        g = self.param_groups[0]
        return ts.export_adam(slices, state[2 * self._side], state[2 * self._side + 1], state[4][self._side], g["lr"], g["betas"], g["eps"],
                              g["weight_decay"], g["decoupled_weight_decay"])

    def check_group(self, group):
        """Raise ValueError, naming both sides, for a param group written under other betas / eps / weight decay than this
        optimiser runs (they are baked into the trainer)."""
        g = self.param_groups[0]
        bad = hip_optim.group_mismatch(group, g["betas"], g["eps"], g["weight_decay"], g["decoupled_weight_decay"])
        if bad:
            raise ValueError("vision4leg_amd: " + bad)

    def load_state_dict(self, sd):
        """From this class or from a real `torch.optim.Adam` / `AdamW` over the same module. Moments go into the trainer's buffers
        in place, the step count to the host side (the next begin() hands it to the device), `lr` into the param group. A state
        written with other betas, eps, weight_decay or the other kind of decay raises (ValueError) before anything is written."""
        net, slices = self._slices()
        m, v, step, group = ts.import_adam(slices, sd, net.total_params)
        self.check_group(group)
        g = self.param_groups[0]
        if self._side:
            self._trainer.load_adam_state(m_vf=m, v_vf=v, steps=(None, step))
        else:
            self._trainer.load_adam_state(m_pf=m, v_pf=v, steps=(step, None))
        g["lr"] = float(group["lr"])


class _StartEpoch(int):
    """`PPO.start_epoch`: the first epoch `train()` runs (0, or the checkpoint's epoch + 1 after `load_checkpoint`) — and, called,
    still the reference's per-epoch hook of that name (rl_algo.py:72-73, 103, 109), which subclasses may override."""

    def __new__(cls, value, hook):
        self = super().__new__(cls, value)
        self._hook = hook
        return self

    def __call__(self):
        return self._hook()


def _dist_world():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_world_size()
    return 1


def exchange_comm_id(dist, device, available, unique_id, id_bytes=_lib.V4L_COMM_ID_BYTES):
    """Bootstrap of the library's own RCCL communicator over an existing process group (any backend): every rank first
    reports whether it can load RCCL (`available()` -> bool) and the ranks AGREE (a min all-reduce) before anyone enters
    ncclCommInitRank — a rank that cannot load the library would otherwise leave the others hanging in the rendezvous.
    Then rank 0's `unique_id()` (128 bytes) is broadcast. -> the id bytes, or None when some rank cannot take part (all ranks
    get None together and fall back to torch.distributed's all-reduce)."""
    on_dev = dist.get_backend() == "nccl"
    kw = {"device": device} if on_dev else {}
    ok = torch.tensor([1 if available() else 0], dtype=torch.int32, **kw)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        return None
    idt = torch.zeros(id_bytes, dtype=torch.uint8, **kw)
    if dist.get_rank() == 0:
        raw = bytes(unique_id())
        if len(raw) != id_bytes:
            raise RuntimeError("vision4leg_amd: communicator id has %d bytes, expected %d" % (len(raw), id_bytes))
        idt.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    dist.broadcast(idt, src=0)
    return bytes(idt.cpu().numpy().tobytes())


def physical_device_index(device, environ=None):
    """The logical device index resolved through the visibility strings (HIP_ / CUDA_VISIBLE_DEVICES select among what
    ROCR_VISIBLE_DEVICES left): '0' and '0,1' both give 0 for logical device 0; an entry that is not a number (a uuid) is kept
    as it is. The tie-breaker of device_identity for runtimes that report one uuid / bus id for several partitions of a GPU."""
    env = os.environ if environ is None else environ
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device() if torch.cuda.is_available() else 0
    for name in (("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"), ("ROCR_VISIBLE_DEVICES",)):
        val = next((env.get(n) for n in name if env.get(n)), None)
        if val is None or not isinstance(idx, int):
            continue
        entries = [e.strip() for e in val.split(",")]
        if idx < len(entries):
            idx = int(entries[idx]) if entries[idx].lstrip("-").isdigit() else entries[idx]
    return idx


def device_identity(device):
    """A 63-bit fingerprint of (host, physical GPU) — equal on two ranks exactly when they drive the same device. Where the
    runtime reports a uuid or PCI ids, (hostname, uuid, PCI ids, physical index) go in — the index RESOLVED through the visibility
    strings, never the strings themselves: two ranks that reach one physical GPU through different visibility strings ('0' and
    '0,1') must get the same fingerprint, or the 'ranks share a GPU' guard is bypassed and ncclCommInitRank is entered with a
    duplicate device; two partitions of one GPU (CPX / SR-IOV guests reporting the same uuid and bus id) must NOT (round-5
    advisor finding). The logical index and the *_VISIBLE_DEVICES strings are the fallback when the runtime reports neither."""
    import hashlib
    import socket
    props = torch.cuda.get_device_properties(device)
    uuid = str(getattr(props, "uuid", "") or "")
    pci = (getattr(props, "pci_domain_id", None), getattr(props, "pci_bus_id", None), getattr(props, "pci_device_id", None))
    if uuid.strip("0-") or any(v is not None for v in pci):
        ident = [socket.gethostname(), uuid, pci, physical_device_index(device)]
    else:
        ident = [socket.gethostname(), (os.environ.get("HIP_VISIBLE_DEVICES"), os.environ.get("ROCR_VISIBLE_DEVICES"),
                                        os.environ.get("CUDA_VISIBLE_DEVICES"), torch.device(device).index)]
    return int.from_bytes(hashlib.sha1(repr(ident).encode()).digest()[:8], "little") >> 1


def _check_update_records(stats, flags, guarded, label=lambda u: "minibatch update %d" % u):
    """The host's rule for the statistics records of a run of updates. stats: [U][V4L_STATS] floats; flags: [U][2] int32
    skipped-step flags (slot 0 = pf, 1 = vf) or None; guarded: the run skipped non-finite optimiser steps
    (PPO(skip_nonfinite_steps=True)). Raises FloatingPointError for the first update whose record counts non-finite statistics
    (slot ST_NONFINITE) unless — guarded only — one of its optimiser steps was skipped; a non-finite ratio next to finite
    gradients still raises. -> (skipped pf steps, skipped vf steps)."""
    stats = np.asarray(stats)
    skipped = np.zeros((len(stats), 2), dtype=np.int64)
    if guarded:
        skipped = np.asarray(flags, dtype=np.int64).reshape(len(stats), 2) != 0
    bad = np.nonzero((stats[:, _lib.ST_NONFINITE] > 0) & ~skipped.any(axis=1))[0]
    if len(bad):  # the device-side tripwire (collector/on_policy.py:102-107 "NaN detected. BOOM")
        raise FloatingPointError("vision4leg_amd: non-finite training statistics in %s: %s"
                                 % (label(int(bad[0])), {k: float(stats[bad[0], j]) for j, k in enumerate(_lib.STAT_KEYS)}))
    return int(skipped[:, 0].sum()), int(skipped[:, 1].sum())


class PPO:
    _call_eps = 1e-5  # the eps the reference's constructor hands optimizer_class (a2c.py:30-40); None: it hands none (reinforce.py:26-29)
    # policies.CategoricalDisPolicy (discrete actions): algo.A2C and algo.Reinforce take it. The reference's PPO reads
    # out['log_std'] (ppo.py:53), which that policy does not return; V-MPO's categorical KL is not built here
    _takes_categorical = False

    def __init__(self, pf, vf, plr=3e-4, vlr=3e-4, optimizer_class=None, entropy_coeff=0.001, clip_para=0.2,
                 opt_epochs=10, clipped_value_loss=False, shuffle=True, tau=None, gae=True, env=None,
                 replay_buffer=None, collector=None, logger=None, grad_clip=None, discount=0.99, num_epochs=3000,
                 batch_size=128, device="cpu", save_interval=100, eval_interval=1, save_dir=None, skip_nonfinite_steps=False,
                 save_train_state=False, resume=None, optimizer_kwargs=None, target_kl=None, desired_kl=None, kl_lr_factor=1.5,
                 kl_lr_min=1e-5, kl_lr_max=1e-2, **kwargs):
        # torch.optim.Adam / AdamW, a functools.partial of either, or "Adam" / "AdamW" + optimizer_kwargs (JSON configs): resolved
        # the way the reference would build it, `optimizer_class(params, lr=..., eps=1e-5)` (a2c.py:30-40); anything else raises
        opt = hip_optim.resolve(optimizer_class, optimizer_kwargs, lr=plr, eps=self._call_eps)
        if getattr(pf, "categorical_head", False) and not self._takes_categorical:  # before anything touches a device
            raise NotImplementedError("vision4leg_amd: %s does not take policies.CategoricalDisPolicy (discrete actions): its loss "
                                      "kernels are Gaussian; the policy runs under algo.A2C and algo.Reinforce"
                                      % type(self).__name__)
        if getattr(pf, "logstd_head", False):  # policies.GaussianContPolicy: before anything touches a device
            forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                      and torch.distributed.is_initialized())
            if _dist_world() > 1 or forced:
                raise NotImplementedError("vision4leg_amd: GaussianContPolicy (log-std from the head) runs in a single process: "
                                          "its data-parallel update (world_size > 1 / V4L_FORCE_DP_PHASES) is not verified")
        # opt-in (config "target_kl"): the KL early stop of an epoch's optimiser steps, decided on the device.
        # None (the reference has no such option): nothing of an update changes.
        if target_kl is not None:  # before anything touches a device
            ok = isinstance(target_kl, (int, float, np.integer, np.floating)) and not isinstance(target_kl, bool)
            if not ok or not (0.0 < float(target_kl) < float("inf")):
                raise ValueError("vision4leg_amd: target_kl must be a positive finite number or None (got %r)" % (target_kl,))
            forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                      and torch.distributed.is_initialized())
            if _dist_world() > 1 or forced:
                raise NotImplementedError("vision4leg_amd: target_kl runs in a single process: data parallel (world_size > 1 / "
                                          "V4L_FORCE_DP_PHASES) each rank would decide the stop on its own shard")
            target_kl = float(target_kl)
        self.target_kl = target_kl
        self.last_kl_stop = None  # (epoch, index of the update that set the latch) of the last stopped run, or None
        self.kl_stops = 0         # runs (epochs) stopped so far; neither is part of the train state
        # opt-in (config "desired_kl", "kl_lr_factor", "kl_lr_min", "kl_lr_max"): legged_gym / rsl_rl's adaptive learning rate,
        # decided on the device after every minibatch update. None: nothing of an update changes.
        nums = {"kl_lr_factor": kl_lr_factor, "kl_lr_min": kl_lr_min, "kl_lr_max": kl_lr_max}  # before anything touches a device
        if desired_kl is not None:
            nums["desired_kl"] = desired_kl
        for key, val in nums.items():
            ok = isinstance(val, (int, float, np.integer, np.floating)) and not isinstance(val, bool)
            if not ok or not (0.0 < float(val) < float("inf")):
                raise ValueError("vision4leg_amd: %s must be a positive finite number%s (got %r)"
                                 % (key, " or None" if key == "desired_kl" else "", val))
        if not float(kl_lr_factor) > 1.0:
            raise ValueError("vision4leg_amd: kl_lr_factor must be > 1 (got %r)" % (kl_lr_factor,))
        if float(kl_lr_min) > float(kl_lr_max):
            raise ValueError("vision4leg_amd: kl_lr_min = %r is above kl_lr_max = %r" % (kl_lr_min, kl_lr_max))
        if desired_kl is not None:
            if target_kl is not None:
                raise ValueError("vision4leg_amd: desired_kl and target_kl are two answers to one estimate (adapt the rates / stop "
                                 "the epoch's steps): a PPO takes one of them")
            forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                      and torch.distributed.is_initialized())
            if _dist_world() > 1 or forced:
                raise NotImplementedError("vision4leg_amd: desired_kl runs in a single process: data parallel (world_size > 1 / "
                                          "V4L_FORCE_DP_PHASES) each rank would adapt the rates on its own shard")
            desired_kl = float(desired_kl)
        self.desired_kl = desired_kl
        self.kl_lr_factor, self.kl_lr_min, self.kl_lr_max = float(kl_lr_factor), float(kl_lr_min), float(kl_lr_max)
        self.lr_changes = {"down": 0, "up": 0}  # decisions -1 / +1 taken so far (not part of the train state)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("vision4leg_amd: PPO needs a GPU device (got %s); there is no CPU path" % self.device)
        # ---- reference attribute surface
        self.target_pf = copy.deepcopy(pf)  # before .to(device), as ppo.py:21
        self.env = env
        self.continuous = not getattr(pf, "categorical_head", False)
        self.replay_buffer = replay_buffer
        self.collector = collector
        self.discount = discount
        self.num_epochs = num_epochs
        self.epoch_frames = getattr(collector, "epoch_frames", None)
        self.batch_size = batch_size
        self.training_update_num = 0
        self.grad_clip = grad_clip
        self.logger = logger
        self.episode_rewards = deque(maxlen=30)
        self.training_episode_rewards = deque(maxlen=30)
        self.save_interval = save_interval
        self.save_dir = save_dir
        if save_dir is not None:
            pathlib.Path(save_dir).mkdir(parents=True, exist_ok=True)
        self.best_eval = None
        self.eval_interval = eval_interval
        self.explore_time = 0
        self.train_time = 0
        self.start = time.time()
        self.shuffle = shuffle
        self.tau = tau
        self.gae = gae
        self.pf = pf
        self.vf = vf
        self.to(self.device)
        self.plr, self.vlr = plr, vlr
        self.optimizer_class = opt.optimizer_class
        self.pf_optimizer = _HipAdam(self.pf.parameters(), plr, opt.eps, opt.betas, opt.weight_decay, opt.decoupled)
        self.vf_optimizer = _HipAdam(self.vf.parameters(), vlr, opt.eps, opt.betas, opt.weight_decay, opt.decoupled)
        self.entropy_coeff = entropy_coeff
        self.clip_para = clip_para
        self.opt_epochs = opt_epochs
        self.clipped_value_loss = clipped_value_loss
        self.sample_key = ["obs", "acts", "advs", "estimate_returns", "values"]
        self.current_epoch = 0
        # resumable training state. save_train_state (config "save_train_state": true): the save_interval and
        # "finish" saves of train() also write train_state_{epoch}.pth; resume (config "resume"): a directory (its newest numbered
        # train_state file) or (directory, epoch) to continue from, loaded at the end of this constructor.
        self.save_train_state = bool(save_train_state)
        self.total_frames = 0
        self.start_epoch = _StartEpoch(0, type(self).start_epoch.__get__(self))
        # opt-in (config "skip_nonfinite_steps": true): an optimiser step whose gradient norm is not finite is skipped on the
        # device — parameters, Adam moments and that optimiser's step count untouched, like torch.cuda.amp.GradScaler.step —
        # instead of writing NaN and raising after the epoch. Off (the reference's behaviour): step, then raise.
        self.skip_nonfinite_steps = bool(skip_nonfinite_steps)
        self.skipped_steps = {"pf": 0, "vf": 0}
        # ---- engine
        self.world_size = _dist_world()
        # the data-parallel update (four phases + one all-reduce per optimiser step) also runs on a 1-rank process group
        # when asked to: that is how the RCCL path is exercised on a single-GPU box (tests/test_gpu_parity.py)
        self.dp_phases = self.world_size > 1 or (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0"
                                                   and torch.distributed.is_available()
                                                   and torch.distributed.is_initialized())
        if self.world_size > 1:
            for p in list(self.pf.parameters()) + list(self.vf.parameters()):
                torch.distributed.broadcast(p.data, src=0)
            atu.copy_model_params_from_to(self.pf, self.target_pf)
            for net in self.networks:  # `.data` writes do not bump the Parameters' version counters
                net.mark_params_changed()
        self.use_graph = os.environ.get("V4L_GRAPH", "1") != "0"
        with torch.cuda.device(self.device):
            self.trainer = HipTrainer(self.pf.hip, self.vf.hip, self.target_pf.hip, batch_size, clip_para,
                                      entropy_coeff, max_grad_norm=0.5, betas=opt.betas, eps=opt.eps,
                                      clipped_value_loss=clipped_value_loss, world_size=self.world_size,
                                      weight_decay=float(opt.weight_decay), decoupled=opt.decoupled)
            # The exchange. Preferred: the library's own RCCL communicator, whose two all-reduces are issued by update_next()
            # INSIDE the captured update graph (no host round trip between backward, all-reduce and Adam). It becomes the
            # schedule only after every rank has passed a self-test of that communicator through the very calls an update
            # makes (_library_comm); otherwise all ranks together keep torch.distributed's all-reduce between four eager
            # phases per update (_update_phases). V4L_DP_COMM = auto (default) | rccl (same, but a failing self-test raises)
            # | torch (never try the library's communicator).
            self.dp_in_library, self.dp_comm_note = False, "single process"
            if self.dp_phases:
                want = os.environ.get("V4L_DP_COMM", "auto").lower()
                if want not in ("auto", "rccl", "torch"):
                    raise ValueError("V4L_DP_COMM must be auto, rccl or torch (got %r)" % want)
                if want == "torch":
                    self.dp_comm_note = "torch.distributed all-reduce between phases (V4L_DP_COMM=torch)"
                else:
                    ok, why = self._library_comm()
                    if ok:
                        self.dp_in_library = True
                        self.dp_phases = False  # update_next() carries the collectives itself
                        self.dp_comm_note = "library RCCL communicator inside the update graph (%s)" % why
                    elif want == "rccl":
                        raise RuntimeError("vision4leg_amd: V4L_DP_COMM=rccl but the library's communicator is not usable: " + why)
                    else:
                        self.dp_comm_note = "torch.distributed all-reduce between phases (library RCCL declined: %s)" % why
        if isinstance(replay_buffer, rb.DeviceOnPolicyReplayBuffer):
            replay_buffer.attach(self.pf.hip, self.device)
        elif replay_buffer is not None:
            replay_buffer.gae_device = self.device
        self._stage = None
        self.pf_optimizer.attach(self.trainer, 0, self.pf)
        self.vf_optimizer.attach(self.trainer, 1, self.vf)
        if resume is not None:
            if isinstance(resume, (str, os.PathLike)):
                prefix, epoch = os.fspath(resume), ts.newest(resume)
                if epoch is None:
                    raise FileNotFoundError("vision4leg_amd: resume=%r holds no train_state_<epoch>.pth" % (resume,))
            else:
                prefix, epoch = resume
            self.load_checkpoint(prefix, epoch)

    # ---- data-parallel bootstrap ---------------------------------------------------------------------
    def _agree(self, ok):
        """True only if `ok` holds on EVERY rank (a MIN all-reduce over the host's process group)."""
        dist = torch.distributed
        kw = {"device": self.device} if dist.get_backend() == "nccl" else {}
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, **kw)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return int(t.item()) == 1

    def _library_comm(self):
        """Bring up the library's RCCL communicator over the host's process group and prove it before relying on it.
        -> (True, what was checked) with the communicator attached on every rank, or (False, why) with none attached on
        any rank. Every decision is taken by all ranks together, so no rank ever waits in a rendezvous alone:
          1. one GPU per rank (RCCL refuses two ranks on a device — the 2-process / 1-GPU test setup);
          2. every rank can load librccl (`exchange_comm_id`), then rank 0's unique id is broadcast and the ranks meet in
             ncclCommInitRank;
          3. v4l_trainer_comm_selftest: both gradient buckets [gradients | tail] carry a rank-dependent integer pattern
             through v4l_sync_grads — eagerly and as a captured graph replayed twice, as update_next() will run it — and
             are checked element by element on the device;
          4. the same pattern through torch.distributed's all-reduce must give the same buffer, and the communicator's
             own rank / size (ncclCommUserRank / ncclCommCount) must equal the process group's."""
        dist = torch.distributed
        tr = self.trainer
        rank, world = dist.get_rank(), dist.get_world_size()
        kw = {"device": self.device} if dist.get_backend() == "nccl" else {}
        mine = torch.tensor([device_identity(self.device)], dtype=torch.int64, **kw)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        if len({int(t.item()) for t in every}) < world:
            return False, "ranks share a GPU; RCCL needs one device per rank"
        comm_id = exchange_comm_id(dist, self.device, HipTrainer.comm_available, HipTrainer.comm_unique_id)
        if comm_id is None:
            return False, "a rank cannot load librccl"
        err = ""
        try:
            tr.comm_init(comm_id, rank, world)
        except RuntimeError as e:
            err = str(e)
        if not self._agree(not err):
            if tr.has_comm:
                tr.comm_destroy()
            return False, "ncclCommInitRank failed on a rank" + (": " + err if err else "")
        try:
            with torch.cuda.stream(tr.stream):
                bad = tr.comm_selftest(graph=self.use_graph)
                if bad:
                    err = "%d elements of the all-reduced self-test pattern are wrong on rank %d" % (bad, rank)
                crank, cworld = tr.comm_info()
                if (crank, cworld) != (rank, world):
                    err = "communicator reports rank %d of %d, the process group %d of %d" % (crank, cworld, rank, world)
                # the critic bucket still holds the library's all-reduced pattern: torch.distributed must produce the same
                n = tr.vf.total_params
                i = torch.arange(n, dtype=torch.int64, device=self.device)
                ref = ((i * 7 + rank * 13) % 251).to(torch.float32)
                got = tr.g_vf.clone()
            tr.stream.synchronize()
            dist.all_reduce(ref)
            if not err and not torch.equal(ref, got):
                err = "library all-reduce and torch.distributed all-reduce disagree on rank %d" % rank
        except RuntimeError as e:
            err = str(e)
        tr.g_vf_bucket.zero_()
        tr.g_pf_bucket.zero_()
        if not self._agree(not err):
            tr.comm_destroy()
            return False, "self-test failed on a rank" + (": " + err if err else "")
        return True, "self-test passed on %d ranks: eager + %s all-reduce of both buckets, cross-checked against " \
                     "torch.distributed" % (world, "graph-replayed" if self.use_graph else "eager-only")

    # ---- reference plumbing ------------------------------------------------------------------------
    @property
    def networks(self):
        return [self.pf, self.vf, self.target_pf]

    @property
    def snapshot_networks(self):
        return [("pf", self.pf), ("vf", self.vf)]

    @property
    def target_networks(self):
        return []

    def to(self, device):
        for net in self.networks:
            net.to(device)

    def start_epoch(self):
        pass

    def finish_epoch(self):
        return {}

    def pretrain(self):
        pass

    def snapshot(self, prefix, epoch):
        """state_dict checkpoints with the reference's file names (rl_algo.py:84-95)."""
        norm = getattr(self.env, "_obs_normalizer", None)
        if norm is not None:
            if hasattr(norm, "to_reference"):
                # the device-resident normaliser (vision4leg_amd.torchrl.env): write what the reference's viewers unpickle
                # (starter/locotransformer_viewer.py:125-147) — an instance of the REFERENCE's Normalizer class — whenever that
                # class is importable (it is under overlay.install(): the reference's torchrl.env is untouched)
                import importlib
                try:
                    ref_cls = importlib.import_module("torchrl.env.base_wrapper").Normalizer
                except ImportError:  # stand-alone use of this package (no reference tree): the pickle then needs this package
                    ref_cls = None
                if ref_cls is not None and ref_cls is not type(norm):
                    norm = norm.to_reference(ref_cls)  # a failing conversion must not silently write an incompatible pickle
            with open(osp.join(prefix, "_obs_normalizer_{}.pkl".format(epoch)), "wb") as f:
                pickle.dump(norm, f)
        for name, network in self.snapshot_networks:
            torch.save(network.state_dict(), osp.join(prefix, "model_{}_{}.pth".format(name, epoch)))

    # ---- resumable training state --------------------------------------------------------
    def train_state(self):
        """Everything of a run that the model files do not hold and that the process would take with it, as tensors, numbers,
        strings, lists and dicts (what torch.load(weights_only=True) reads). Reads the Adam moments back: one synchronise."""
        from ....engine import COMPUTE_NAMES
        coll = self.collector
        with torch.cuda.device(self.device):
            cuda_rng = torch.cuda.get_rng_state(self.device)
            return {
                "format_version": ts.FORMAT_VERSION,
                "pf_optimizer": self.pf_optimizer.state_dict(),
                "vf_optimizer": self.vf_optimizer.state_dict(),
                "epoch": int(self.current_epoch),  # the last completed epoch
                "total_frames": int(self.total_frames),
                "training_update_num": int(self.training_update_num),
                "best_eval": None if self.best_eval is None else float(self.best_eval),
                "episode_rewards": ts.plain_rewards(self.episode_rewards),
                "training_episode_rewards": ts.plain_rewards(self.training_episode_rewards),
                "skipped_steps": {k: int(v) for k, v in self.skipped_steps.items()},
                "f16_saturated": float(self.f16_saturated),
                "compute": COMPUTE_NAMES[self.pf.hip.compute],
                "net_kinds": {"pf": int(self.pf.hip.kind), "vf": int(self.vf.hip.kind)},
                "rng": {"numpy": ts.pack_numpy_rng(), "torch_cpu": torch.get_rng_state(), "torch_cuda": cuda_rng},
                "collector": {"current_step": ts.optional_tensor(getattr(coll, "current_step", None)),
                              "train_rew": ts.optional_tensor(getattr(coll, "train_rew", None))},
            }

    def save_checkpoint(self, prefix, epoch):
        """snapshot(prefix, epoch) — the reference's files, names and contents unchanged — plus train_state_{epoch}.pth: both
        optimisers in torch.optim.Adam's state_dict format, the schedule position, counters and RNG streams. Data parallel:
        every rank reads its state back (the ranks hold the same), rank 0 writes."""
        state = self.train_state()
        if self.world_size > 1 and torch.distributed.get_rank() != 0:
            return
        self.snapshot(prefix, epoch)
        tmp = ts.path(prefix, epoch) + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, ts.path(prefix, epoch))  # a process killed while writing leaves the previous file whole

    def _check_model_file(self, name, network, sd, state):
        """A checkpoint of another net geometry: raise with the first mismatching parameter, before anything is overwritten."""
        have = {k: tuple(v.shape) for k, v in network.state_dict().items()}
        got = {k: tuple(v.shape) for k, v in sd.items()}
        bad = next((k for k in got if have.get(k) != got[k]), None) or next((k for k in have if k not in got), None)
        if bad is not None:
            raise RuntimeError("vision4leg_amd: checkpoint does not fit this %s net: parameter %s is %s in the file and %s here "
                               "(file: net kinds %s, compute %s; here: kind %d)"
                               % (name, bad, got.get(bad, "missing"), have.get(bad, "missing"), state.get("net_kinds"),
                                  state.get("compute"), network.hip.kind))

    def load_checkpoint(self, prefix, epoch, restore_rng=True, restore_collector=False):
        """Continue from save_checkpoint(prefix, epoch): parameters, both Adam moment sets and step counts, the schedule position
        (train() goes on at the file's epoch + 1), counters and — restore_rng — numpy's, torch's CPU and this device's generator
        states. A file written in another compute mode loads (the masters are fp32); another net geometry raises. The simulator
        is not part of the file: the run goes on from env.reset(), which is why the collector's per-episode step counts and
        partial returns are in the file but only put back on request (restore_collector: for a caller that restores its env)."""
        state = ts.load(prefix, epoch)
        files = {}
        for name, network in self.snapshot_networks:
            files[name] = torch.load(osp.join(prefix, "model_{}_{}.pth".format(name, epoch)), map_location="cpu", weights_only=True)
            self._check_model_file(name, network, files[name], state)
        for opt, key in ((self.pf_optimizer, "pf_optimizer"), (self.vf_optimizer, "vf_optimizer")):
            for group in state[key]["param_groups"]:  # a file written under another optimiser setting: before anything is overwritten
                opt.check_group(group)
        with torch.cuda.device(self.device):
            for name, network in self.snapshot_networks:
                network.load_state_dict(files[name])
            atu.copy_model_params_from_to(self.pf, self.target_pf)
            for net in self.networks:
                net.mark_params_changed()
            self._load_normalizer(osp.join(prefix, "_obs_normalizer_{}.pkl".format(epoch)))
            self.pf_optimizer.load_state_dict(state["pf_optimizer"])
            self.vf_optimizer.load_state_dict(state["vf_optimizer"])
            self.training_update_num = int(state["training_update_num"])
            self.trainer.step = self.training_update_num  # updates run, skipped steps included
            if self.world_size > 1:
                self._agree_on_adam_state()
            if restore_rng:
                np.random.set_state(ts.unpack_numpy_rng(state["rng"]["numpy"]))
                torch.set_rng_state(state["rng"]["torch_cpu"])
                torch.cuda.set_rng_state(state["rng"]["torch_cuda"], self.device)
        self.total_frames = int(state["total_frames"])
        self.best_eval = state["best_eval"]
        self.episode_rewards = deque(ts.restore_rewards(state["episode_rewards"]), maxlen=30)
        self.training_episode_rewards = deque(ts.restore_rewards(state["training_episode_rewards"]), maxlen=30)
        self.skipped_steps = {k: int(v) for k, v in state["skipped_steps"].items()}
        if state["f16_saturated"]:
            self.f16_saturated = float(state["f16_saturated"])
        if restore_collector:
            for key, value in state["collector"].items():
                if value is not None:
                    setattr(self.collector, key, value.numpy().copy())
        self.current_epoch = int(state["epoch"])
        self.start_epoch = _StartEpoch(self.current_epoch + 1, self.start_epoch._hook)
        return state

    def _load_normalizer(self, path):
        norm = getattr(self.env, "_obs_normalizer", None)
        if norm is None or not osp.exists(path):
            return
        with open(path, "rb") as f:  # written by snapshot(): this package's or the reference's Normalizer
            saved = pickle.load(f)
        if hasattr(norm, "load_state"):  # the device-resident normaliser: in place, its buffers keep their addresses
            norm.load_state(saved.state() if hasattr(saved, "state") else type(norm).from_reference(saved, norm.device).state())
        else:
            self.env._obs_normalizer = saved

    def _agree_on_adam_state(self):
        """Data parallel: every rank read the file itself; one MIN all-reduce over [x | -x] (min and -max of each entry) shows
        whether the step counts and a sum over the loaded moments are the same on all ranks. Raises on every rank if not."""
        dist = torch.distributed
        m_pf, v_pf, m_vf, v_vf, steps = self.trainer.adam_state()
        x = torch.stack([torch.tensor(float(s), dtype=torch.float64, device=self.device) for s in steps]
                        + [b.double().sum() for b in (m_pf, v_pf, m_vf, v_vf)])
        t = torch.cat([x, -x])
        if dist.get_backend() != "nccl":
            t = t.cpu()
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        lo, hi = t[:6], -t[6:]
        if not torch.equal(lo, hi):
            raise RuntimeError("vision4leg_amd: the ranks loaded different optimiser states (step counts / moment sums, smallest "
                               "%s, largest %s)" % (lo.tolist(), hi.tolist()))

    # ---- epoch ---------------------------------------------------------------------------------------
    def process_epoch_samples(self):
        """last_value = vf(next_obs[T-1]) * (1 - terminal) then GAE — or, gae=False, discounted rewards (on_rl_algo.py:23-34)."""
        sample = self.replay_buffer.last_sample(["next_obs", "terminals", "time_limits"])
        last_ob = sample["next_obs"]
        if not isinstance(last_ob, torch.Tensor):
            last_ob = torch.from_numpy(np.ascontiguousarray(last_ob, dtype=np.float32))
        last_value = self.vf(last_ob.to(self.device, torch.float32)).cpu().numpy()
        last_value = last_value * (1 - sample["terminals"])
        if self.gae:
            self.replay_buffer.generalized_advantage_estimation(last_value, self.discount, self.tau)
        else:  # on_rl_algo.py:29-33
            self.replay_buffer.discount_reward(last_value, self.discount)

    def update_per_epoch(self):
        with torch.cuda.device(self.device):
            self.process_epoch_samples()
            if getattr(self, "desired_kl", None) is None:
                atu.update_linear_schedule(self.pf_optimizer, self.current_epoch, self.num_epochs, self.plr)
                atu.update_linear_schedule(self.vf_optimizer, self.current_epoch, self.num_epochs, self.vlr)
            # (desired_kl: the optimisers' rates are the ones the device left after the last run — rsl_rl's schedule = "adaptive")
            self.trainer.sync_target()  # copy_model_params_from_to(pf, target_pf), ppo.py:34
            if isinstance(self.replay_buffer, rb.DeviceOnPolicyReplayBuffer):
                self._update_epoch_resident()
                return
            u = 0
            for _ in range(self.opt_epochs):
                for batch in self.replay_buffer.one_iteration(self.batch_size, self.sample_key, self.shuffle):
                    infos = self.update(batch)
                    self.logger.add_update_info(infos)
                    if infos.get("kl_stop"):  # target_kl: the update that reported the stop is the epoch's last (both loops end)
                        self._note_kl_stop(u)
                        return
                    u += 1

    def _epoch_rowidx(self, passes):
        """The row lists of all minibatches of an epoch, `passes` times over the samples -> int32 [U][n] device tensor."""
        batches = [b["rowidx"] for _ in range(passes)
                   for b in self.replay_buffer.one_iteration(self.batch_size, self.sample_key, self.shuffle)]
        return torch.from_numpy(np.stack(batches)).to(self.device)  # one upload per epoch

    def _update_epoch_resident(self):
        state, image, acts, advs, rets, vals, logp = self.replay_buffer.device_rollout()
        ro = HipTrainer.rollout(state, image, acts, advs, rets, vals, logp)
        rowidx = self._epoch_rowidx(self.opt_epochs)
        U = len(rowidx)
        stats = torch.zeros(U, _lib.V4L_STATS, dtype=torch.float32, device=self.device)
        self.run_updates(ro, rowidx, stats)
        flags = kl = ad = None
        if self.desired_kl is not None:  # records, flags and the [U][4] columns share one allocation: still one device->host copy
            rec = self._rec_buf.cpu()
            host = rec[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS).numpy()
            if self.skip_nonfinite_steps:
                flags = rec[U * _lib.V4L_STATS:U * (_lib.V4L_STATS + 2)].view(torch.int32).view(U, 2).numpy()
            ad = rec[U * (_lib.V4L_STATS + 2):].view(U, 4).numpy()
        elif self.target_kl is not None:  # records, flags and KL columns share one allocation: still one device->host copy
            rec = self._rec_buf.cpu()
            host = rec[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS).numpy()
            if self.skip_nonfinite_steps:
                flags = rec[U * _lib.V4L_STATS:U * (_lib.V4L_STATS + 2)].view(torch.int32).view(U, 2).numpy()
            kl = rec[U * (_lib.V4L_STATS + 2):].view(U, 2).numpy()
        elif self.skip_nonfinite_steps:  # records and flags share one allocation: still one device->host copy
            rec = self._rec_buf.cpu()
            host = rec[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS).numpy()
            flags = rec[U * _lib.V4L_STATS:].view(torch.int32).view(U, 2).numpy()
        else:
            host = stats.cpu().numpy()  # the only device->host sync of the epoch's updates
        spf, svf = _check_update_records(host, flags, self.skip_nonfinite_steps,
                                         lambda u: "minibatch update %d of epoch %d" % (u, self.current_epoch))
        self._note_skipped(spf, svf)
        self._note_f16_saturation(float(host[:, _lib.ST_F16_SAT].sum()))
        for u, row in enumerate(host):
            self.logger.add_update_info(self._info(row, None if flags is None else flags[u], None if kl is None else kl[u],
                                                   None if ad is None else ad[u]))
            if ad is not None:
                self._note_lr_decision(ad[u][1])
            if kl is not None and kl[u][1] != 0:  # the updates after the stop changed nothing: the logger gets none of them
                self._note_kl_stop(u)
                break

    def _info(self, row, flags, kl=None, adapt=None):
        """The logger's info dict of one update: the 18 reference keys, with the guard on skipped/pf and skipped/vf (0 / 1), with
        target_kl approx_kl and kl_stop (0 / 1), and with desired_kl approx_kl, lr_decision (-1 / 0 / 1), lr/pf and lr/vf (the
        rates in force after the update, as the device's record holds them: floats)."""
        info = {k: float(row[j]) for j, k in enumerate(_lib.STAT_KEYS)}
        if flags is not None:
            info["skipped/pf"], info["skipped/vf"] = int(flags[0] != 0), int(flags[1] != 0)
        if kl is not None:
            info["approx_kl"], info["kl_stop"] = float(kl[0]), int(kl[1] != 0)
        if adapt is not None:
            info["approx_kl"], info["lr_decision"] = float(adapt[0]), int(adapt[1])
            info["lr/pf"], info["lr/vf"] = float(adapt[2]), float(adapt[3])
        return info

    def _note_lr_decision(self, d):
        if d < 0:
            self.lr_changes["down"] += 1
        elif d > 0:
            self.lr_changes["up"] += 1

    def _take_device_lrs(self):
        """desired_kl: after a run the optimisers carry the rates the device left, as doubles (HipTrainer.lrs()): the next run's
        begin() is handed those, and state_dict() saves them."""
        lr_pf, lr_vf = self.trainer.lrs()
        self.pf_optimizer.param_groups[0]["lr"] = lr_pf
        self.vf_optimizer.param_groups[0]["lr"] = lr_vf

    def _note_kl_stop(self, u):
        self.last_kl_stop = (self.current_epoch, int(u))
        self.kl_stops += 1

    def _note_skipped(self, spf, svf):
        if spf or svf:
            import warnings
            self.skipped_steps["pf"] += spf
            self.skipped_steps["vf"] += svf
            warnings.warn("vision4leg_amd: skipped %d policy and %d critic optimiser step(s) whose gradient norm was not finite "
                          "(epoch %d; PPO.skipped_steps keeps the totals: %s)" % (spf, svf, self.current_epoch, self.skipped_steps),
                          RuntimeWarning)

    f16_saturated = 0.0  # V4L_COMPUTE=f16: loss-gradient elements clamped at +-V4L_F16_GRAD_CLAMP so far (include/v4l_hip.h, record slot 23)

    def _note_f16_saturation(self, count):
        """f16 compute mode: the loss-gradient rows enter the backward scaled by a power of two and clamped inside half's range.
        A clamped element is a per-sample gradient clip the reference does not have: counted, and reported once."""
        if count > 0:
            if self.f16_saturated == 0:
                import warnings
                warnings.warn("vision4leg_amd: %d loss-gradient element(s) of an f16 update exceeded +-%g after scaling and were "
                              "clamped (record slot %d; PPO.f16_saturated keeps the total). Returns / advantages of that size "
                              "want V4L_COMPUTE=bf16." % (int(count), 32768.0, _lib.ST_F16_SAT), RuntimeWarning)
            self.f16_saturated += count

    def _run_updates_kl(self, ro, rowidx, stats, skip, kl):
        """run_updates with target_kl: the armed run (HipTrainer.kl_arm / kl_update_run, graphs of their own), by run_updates'
        switches. Records, guard flags and the KL columns [U][2] (approx_kl, latch) share one allocation."""
        tr = self.trainer
        U, n = rowidx.shape
        if getattr(self, "_rowidx_buf", None) is None or self._rowidx_buf.shape != rowidx.shape:
            self._rowidx_buf = torch.empty_like(rowidx)
            self._rec_buf = torch.zeros(U * (_lib.V4L_STATS + 4), dtype=torch.float32, device=self.device)
            self._stats_buf = self._rec_buf[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS)
            self._skip_buf = self._rec_buf[U * _lib.V4L_STATS:U * (_lib.V4L_STATS + 2)].view(torch.int32).view(U, 2)
            self._kl_buf = self._rec_buf[U * (_lib.V4L_STATS + 2):].view(U, 2)
        self._rowidx_buf.copy_(rowidx)
        cur = torch.cuda.current_stream(self.device)
        tr.stream.wait_stream(cur)
        with torch.cuda.stream(tr.stream):
            tr._pre(n)
            tr.begin(self._rowidx_buf, self._stats_buf, self.pf_optimizer.lr, self.vf_optimizer.lr,
                     self._skip_buf if self.skip_nonfinite_steps else None)
            tr.kl_arm(self._kl_buf, self.target_kl)
            self.training_update_num += U
            if self.use_graph and os.environ.get("V4L_EPOCH_GRAPH", "1") != "0":
                tr.kl_update_run(ro, n, U, graph=True)
            else:
                for _ in range(U):
                    tr.kl_update_next(ro, n, graph=self.use_graph)
            stats.copy_(self._stats_buf)
            if skip is not None:
                skip.copy_(self._skip_buf)
            if kl is not None:
                kl.copy_(self._kl_buf)
        cur.wait_stream(tr.stream)

    def _run_updates_kl_adapt(self, ro, rowidx, stats, skip, kl):
        """run_updates with desired_kl: the armed run (HipTrainer.kl_adapt_arm / kl_adapt_update_run, graphs of their own), by
        run_updates' switches. Records, guard flags and the columns [U][4] (approx_kl, decision, lr_pf, lr_vf) share one
        allocation. Afterwards the optimisers carry the rates the device left (read back as doubles)."""
        tr = self.trainer
        U, n = rowidx.shape
        if getattr(self, "_rowidx_buf", None) is None or self._rowidx_buf.shape != rowidx.shape:
            self._rowidx_buf = torch.empty_like(rowidx)
            self._rec_buf = torch.zeros(U * (_lib.V4L_STATS + 6), dtype=torch.float32, device=self.device)
            self._stats_buf = self._rec_buf[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS)
            self._skip_buf = self._rec_buf[U * _lib.V4L_STATS:U * (_lib.V4L_STATS + 2)].view(torch.int32).view(U, 2)
            self._kl_buf = self._rec_buf[U * (_lib.V4L_STATS + 2):].view(U, 4)
        self._rowidx_buf.copy_(rowidx)
        cur = torch.cuda.current_stream(self.device)
        tr.stream.wait_stream(cur)
        with torch.cuda.stream(tr.stream):
            tr._pre(n)
            tr.begin(self._rowidx_buf, self._stats_buf, self.pf_optimizer.lr, self.vf_optimizer.lr,
                     self._skip_buf if self.skip_nonfinite_steps else None)
            tr.kl_adapt_arm(self._kl_buf, self.desired_kl, self.kl_lr_factor, self.kl_lr_min, self.kl_lr_max)
            self.training_update_num += U
            if self.use_graph and os.environ.get("V4L_EPOCH_GRAPH", "1") != "0":
                tr.kl_adapt_update_run(ro, n, U, graph=True)
            else:
                for _ in range(U):
                    tr.kl_adapt_update_next(ro, n, graph=self.use_graph)
            stats.copy_(self._stats_buf)
            if skip is not None:
                skip.copy_(self._skip_buf)
            if kl is not None:
                kl.copy_(self._kl_buf)
            self._take_device_lrs()
        cur.wait_stream(tr.stream)

    def run_updates(self, ro, rowidx, stats, skip=None, kl=None):
        """All minibatch updates of an epoch: rowidx [U][n] int32 (device), stats [U][V4L_STATS] (device); skip: None or an
        int32 [U][2] device tensor that receives the guard's skipped-step flags (skip_nonfinite_steps); kl (target_kl only): None
        or a float32 [U][2] device tensor that receives (approx_kl, latch) per update — every optimiser step after the update that
        set the latch is skipped on the device; the launches still run (a stop saves no GPU time here).
        The whole run is ONE hipGraph replay on the trainer's stream (round 6; one replay per update with V4L_EPOCH_GRAPH=0) — on one
        GPU, and data-parallel with the library's own communicator (V4L_DP_COMM=rccl: both all-reduces are nodes of that graph). With torch.distributed doing the exchange
        (the data-parallel default) an update is four eager phases with one all-reduce per optimiser step between them.
        With desired_kl, kl is None or a float32 [U][4] device tensor that receives (approx_kl, decision, lr_pf, lr_vf) per update,
        and the optimisers' rates are afterwards those the device left."""
        if self.desired_kl is not None:
            return self._run_updates_kl_adapt(ro, rowidx, stats, skip, kl)
        if self.target_kl is not None:
            return self._run_updates_kl(ro, rowidx, stats, skip, kl)
        tr = self.trainer
        U, n = rowidx.shape
        # the captured graph is keyed on these addresses: keep them stable from epoch to epoch
        if getattr(self, "_rowidx_buf", None) is None or self._rowidx_buf.shape != rowidx.shape:
            self._rowidx_buf = torch.empty_like(rowidx)
            # [U][V4L_STATS] records, then the guard's [U][2] int32 skipped-step flags in the same allocation
            self._rec_buf = torch.zeros(U * (_lib.V4L_STATS + 2), dtype=torch.float32, device=self.device)
            self._stats_buf = self._rec_buf[:U * _lib.V4L_STATS].view(U, _lib.V4L_STATS)
            self._skip_buf = self._rec_buf[U * _lib.V4L_STATS:].view(torch.int32).view(U, 2)
        self._rowidx_buf.copy_(rowidx)
        cur = torch.cuda.current_stream(self.device)
        tr.stream.wait_stream(cur)
        with torch.cuda.stream(tr.stream):
            tr.begin(self._rowidx_buf, self._stats_buf, self.pf_optimizer.lr, self.vf_optimizer.lr,
                     self._skip_buf if self.skip_nonfinite_steps else None)
            if not self.dp_phases and self.use_graph and os.environ.get("V4L_EPOCH_GRAPH", "1") != "0":
                # the whole epoch loop (ppo.py:28-40) as ONE hipGraph replay (round 6); V4L_EPOCH_GRAPH=0: one replay per update
                self.training_update_num += U
                tr.update_run(ro, n, U, graph=True)
            else:
                for _ in range(U):
                    self.training_update_num += 1
                    if not self.dp_phases:
                        tr.update_next(ro, n, graph=self.use_graph)
                    else:
                        self._update_phases(ro, n)
            stats.copy_(self._stats_buf)
            if skip is not None:
                skip.copy_(self._skip_buf)
        cur.wait_stream(tr.stream)

    def _update_phases(self, ro, n):
        """The exchange done by torch.distributed (V4L_DP_COMM=torch): four eager phases, the buckets [gradients | tail]
        all-reduced between them. (The guard's decision is taken on the all-reduced buckets: every rank skips the same steps.)"""
        dist = torch.distributed
        tr = self.trainer
        tr.critic_grads(ro, n)
        tr.bucket_tail(1, 1, self.world_size)
        dist.all_reduce(tr.g_vf_bucket)  # sum over env shards: critic grads + advantage moments + vf_loss share
        tr.bucket_tail(1, 0, self.world_size)
        tr.critic_step()
        tr.actor_grads(ro, n)
        tr.bucket_tail(0, 1, self.world_size)
        dist.all_reduce(tr.g_pf_bucket)
        tr.bucket_tail(0, 0, self.world_size)
        tr.actor_step()

    def _upload_batch(self, batch, keys):
        """A reference-style host batch onto the device: batch["obs"] ingested into the staging rollout `_stage` ((re)allocated
        for its row count), batch[k] for k in keys as fresh float32 tensors ("acts" [n][A], the others [n]). -> n, those tensors."""
        if "rowidx" in batch:
            raise RuntimeError("device-resident batches are consumed by update_per_epoch")
        if getattr(self.pf, "categorical_head", False) and "acts" in keys:  # action indices: checked on the host, before any upload
            acts, K = np.asarray(batch["acts"]), self.pf.output_dim
            if not (np.isfinite(acts).all() and (acts == np.floor(acts)).all() and (acts >= 0).all() and (acts < K).all()):
                raise ValueError("vision4leg_amd: CategoricalDisPolicy: batch['acts'] must hold integer action indices in "
                                 "[0, %d)" % K)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        obs = up(batch["obs"])
        n = obs.shape[0]
        net = self.pf.hip
        net.ensure_bound()
        if self._stage is None or self._stage[0].shape[0] != n:
            self._stage = net.alloc_rollout(n, self.device)
        net.ingest(obs, self._stage[0], self._stage[1])
        return n, [up(batch[k]).reshape((n, -1) if k == "acts" else n) for k in keys]

    def update(self, batch):
        """One minibatch update from a reference-style host batch (ppo.py:125-153). Returns the 18-key info (plus skipped/* with
        the guard, approx_kl and kl_stop with target_kl: here a run is this one update, so kl_stop = 1 says that its policy step
        was skipped and that the caller's loops over the epoch's minibatches should end, as update_per_epoch's do)."""
        dev = self.device
        with torch.cuda.device(dev):
            n, arrays = self._upload_batch(batch, ("acts", "advs", "estimate_returns", "values"))
            self.training_update_num += 1
            ro = HipTrainer.rollout(self._stage[0], self._stage[1], *arrays)
            stats = torch.zeros(1, _lib.V4L_STATS, dtype=torch.float32, device=dev)
            skip = torch.zeros(1, 2, dtype=torch.int32, device=dev) if self.skip_nonfinite_steps else None
            kl = ad = None
            tr = self.trainer
            if self.desired_kl is not None:  # a run of one update armed with the adaptive rates, eager like the ones below
                ad = torch.zeros(1, 4, dtype=torch.float32, device=dev)
                tr._pre(n)
                tr.begin(None, stats, self.pf_optimizer.lr, self.vf_optimizer.lr, skip)
                tr.kl_adapt_arm(ad, self.desired_kl, self.kl_lr_factor, self.kl_lr_min, self.kl_lr_max)
                tr.kl_adapt_update_next(ro, n, graph=False)
                self._take_device_lrs()  # the next update(batch) opens with them
            elif self.target_kl is not None:  # a run of one armed update, eager like the one below
                kl = torch.zeros(1, 2, dtype=torch.float32, device=dev)
                tr._pre(n)
                tr.begin(None, stats, self.pf_optimizer.lr, self.vf_optimizer.lr, skip)
                tr.kl_arm(kl, self.target_kl)
                tr.kl_update_next(ro, n, graph=False)
            elif not self.dp_phases:
                tr.update(ro, None, n, self.pf_optimizer.lr, self.vf_optimizer.lr, stats, skip)
            else:
                tr._pre(n)
                tr.begin(None, stats, self.pf_optimizer.lr, self.vf_optimizer.lr, skip)
                self._update_phases(ro, n)
            host = stats[0].cpu().numpy()
            flags = skip.cpu().numpy() if skip is not None else None
            klh = kl.cpu().numpy() if kl is not None else None
            adh = ad.cpu().numpy() if ad is not None else None
        if adh is not None:
            self._note_lr_decision(adh[0][1])
        # the device-side tripwire, as in _update_epoch_resident
        spf, svf = _check_update_records(host[None], flags, self.skip_nonfinite_steps,
                                         lambda u: "minibatch update %d" % self.training_update_num)
        self._note_skipped(spf, svf)
        self._note_f16_saturation(float(host[_lib.ST_F16_SAT]))
        return self._info(host, None if flags is None else flags[0], None if klh is None else klh[0],
                          None if adh is None else adh[0])

    # ---- outer loop (rl_algo.py:97-168) ----------------------------------------------------------------
    def train(self):
        self.pretrain()
        first = int(self.start_epoch)  # 0, or the epoch after a loaded checkpoint's (load_checkpoint)
        total_frames = self.total_frames if first else getattr(self, "pretrain_frames", 0)
        save = self.save_checkpoint if self.save_train_state else self.snapshot
        self.start_epoch()
        for epoch in range(first, self.num_epochs):
            self.current_epoch = epoch
            self.start_epoch()
            t0 = time.time()
            training_epoch_info = self.collector.train_one_epoch()
            for reward in training_epoch_info["train_rewards"]:
                self.training_episode_rewards.append(reward)
            self.explore_time += time.time() - t0
            t0 = time.time()
            self.update_per_epoch()
            torch.cuda.synchronize(self.device)
            self.train_time += time.time() - t0
            finish_epoch_info = self.finish_epoch()
            total_frames += self.epoch_frames
            self.total_frames = total_frames
            if epoch % self.eval_interval == 0:
                t0 = time.time()
                eval_infos = self.collector.eval_one_epoch()
                eval_time = time.time() - t0
                infos = {}
                for reward in eval_infos["eval_rewards"]:
                    self.episode_rewards.append(reward)
                mean_eval = np.mean(eval_infos["eval_rewards"])
                if self.best_eval is None or mean_eval > self.best_eval:
                    self.best_eval = mean_eval
                    self.snapshot(self.save_dir, "best")
                    print("Best Saved: {:.5f},  EPoch: {}".format(mean_eval, epoch))
                del eval_infos["eval_rewards"]
                infos["Running_Average_Rewards"] = np.mean(self.episode_rewards)
                infos["Train_Epoch_Reward"] = training_epoch_info["train_epoch_reward"]
                infos["Running_Training_Average_Rewards"] = np.mean(self.training_episode_rewards)
                infos["Explore_Time"] = self.explore_time
                infos["Train___Time"] = self.train_time
                infos["Eval____Time"] = eval_time
                self.explore_time = 0
                self.train_time = 0
                infos.update(eval_infos)
                infos.update(finish_epoch_info)
                self.logger.add_epoch_info(epoch, total_frames, time.time() - self.start, infos)
                self.start = time.time()
            if epoch % self.save_interval == 0:
                save(self.save_dir, epoch)
        save(self.save_dir, "finish")
        self.collector.terminate()
