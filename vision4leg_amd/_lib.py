"""ctypes binding of libv4l_hip.so (C ABI declared in include/v4l_hip.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("V4L_LIB", os.path.join(_HERE, "libv4l_hip.so"))  # V4L_LIB: diagnostic builds only
SRC_DIR = os.path.join(_HERE, "csrc")

V4L_F32, V4L_BF16, V4L_F16 = 0, 1, 2
V4L_NET_MLP, V4L_NET_CNN, V4L_NET_LOCO, V4L_NET_CNN_VIS, V4L_NET_LOCO_VIS = 0, 1, 2, 3, 4
V4L_ACT_RELU, V4L_ACT_TANH = 0, 1
V4L_LOGSTD_NONE, V4L_LOGSTD_PARAM, V4L_LOGSTD_HEAD = 0, 1, 2  # NetCfg.has_logstd: value net / logstd parameter / log sigma from the head
V4L_MAX_HIDDEN = 4
V4L_STATS = 24
ST_NONFINITE = 22   # record slot: number of NaN / Inf among the 18 logged scalars of an update
ST_F16_SAT = 23     # record slot: V4L_F16 — loss-gradient elements of the update clamped at +-V4L_F16_GRAD_CLAMP
V4L_OUT_LD = 16
V4L_MAX_ACT = 16   # widest action vector of a policy (include/v4l_hip.h)
V4L_VMPO_STATS = 12   # floats per update in the V-MPO record (include/v4l_hip.h)
V4L_VMPO_STATE = 7    # doubles of v4l_trainer_vmpo_state: eta, alpha, exp_avg x 2, exp_avg_sq x 2, step
V4L_A2C_STATS = 16    # floats per update in the A2C record (include/v4l_hip.h)
V4L_REINFORCE_STATS = 12   # floats per update in the REINFORCE record (include/v4l_hip.h)
V4L_BUCKET_TAIL = 8   # scalars behind the gradients of an all-reduce bucket
V4L_COMM_ID_BYTES = 128
V4L_CAST_MAX_THREADS = 64   # most host threads that cast one job's rows (include/v4l_hip.h)


def clamp_cast_threads(threads):
  """The thread count handed to v4l_actor_step_rows: any integer -> [1, V4L_CAST_MAX_THREADS]."""
  return max(1, min(int(threads), V4L_CAST_MAX_THREADS))

# order of the 18 logger keys inside a stats record (torchrl/algo/on_policy/ppo.py:77-92,122-123,142-145)
STAT_KEYS = [
  "advs/mean", "advs/std", "advs/max", "advs/min", "Training/vf_loss", "grad_norm/vf",
  "Training/policy_loss", "logprob/mean", "logprob/std", "logprob/max", "logprob/min",
  "log_std/mean", "log_std/std", "log_std/max", "log_std/min", "ratio/max", "ratio/min",
  "grad_norm/pf",
]


class NetCfg(C.Structure):
  _fields_ = [
    ("kind", C.c_int), ("compute", C.c_int), ("state_dim", C.c_int), ("out_dim", C.c_int),
    ("in_channels", C.c_int), ("img_hw", C.c_int), ("n_enc_hidden", C.c_int),
    ("enc_hidden", C.c_int * V4L_MAX_HIDDEN), ("visual_dim", C.c_int), ("token_dim", C.c_int),
    ("n_layers", C.c_int), ("ff_dim", C.c_int), ("n_head_hidden", C.c_int),
    ("head_hidden", C.c_int * V4L_MAX_HIDDEN), ("has_logstd", C.c_int), ("tanh_action", C.c_int), ("max_pool", C.c_int),
    ("token_norm", C.c_int), ("pytorch_encoder", C.c_int), ("activation", C.c_int),
  ]


class PPOHyper(C.Structure):
  _fields_ = [
    ("clip_para", C.c_float), ("entropy_coeff", C.c_float), ("max_grad_norm", C.c_float),
    ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
    ("clipped_value_loss", C.c_int), ("world_size", C.c_int),
    ("weight_decay", C.c_double), ("decoupled_weight_decay", C.c_int),
  ]


# the V-MPO record's logger keys, in record order (torchrl/algo/on_policy/v_mpo.py:119-132); slots 7, 8: d(loss)/d(eta), d(alpha)
VMPO_STAT_KEYS = ["Training/alpha_loss", "Training/alpha", "Training/eta", "KL/mean", "KL/std", "KL/max", "KL/min"]
# the 19 keys VMPO.update returns, in the reference's order: 12 of the PPO record (no log_std/*, no ratio/*) + the 7 above
VMPO_INFO_KEYS = (STAT_KEYS[:7] + VMPO_STAT_KEYS[:3] + STAT_KEYS[7:11] + VMPO_STAT_KEYS[3:] + ["grad_norm/pf"])


# the A2C record's first 12 slots = the keys A2C.update returns, in the reference's order (torchrl/algo/on_policy/a2c.py:89-105)
A2C_INFO_KEYS = ["Training/policy_loss", "Training/vf_loss", "v_pred/mean", "v_pred/std", "v_pred/max", "v_pred/min",
                 "std/mean", "std/std", "std/max", "std/min", "ent", "log_prob"]
# the 8 of them a categorical policy leaves: the reference logs std/* only `if 'std' in out` (a2c.py:63-65,97-102)
A2C_CAT_INFO_KEYS = [k for k in A2C_INFO_KEYS if not k.startswith("std/")]

# the REINFORCE record's first 10 slots = the keys Reinforce.update returns, in the reference's order
# (torchrl/algo/on_policy/reinforce.py:43-74)
REINFORCE_INFO_KEYS = ["advs/mean", "advs/std", "advs/max", "advs/min", "Training/policy_loss", "ent",
                       "logprob/mean", "logprob/std", "logprob/max", "logprob/min"]


class VMPOHyper(C.Structure):
  _fields_ = [("eta_eps", C.c_double), ("alpha_eps", C.c_double), ("eta0", C.c_double), ("alpha0", C.c_double),
              ("lr_scale", C.c_double)]


class Rollout(C.Structure):
  _fields_ = [
    ("state_dev", C.c_void_p), ("image_dev", C.c_void_p), ("acts_dev", C.c_void_p),
    ("advs_dev", C.c_void_p), ("rets_dev", C.c_void_p), ("values_dev", C.c_void_p), ("logp_old_dev", C.c_void_p),
  ]


def build_command(out=LIB_PATH):
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  return [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
          os.path.join(SRC_DIR, "v4l_hip.hip"), "-o", out]


def build(force=False):
  """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
  srcs = [os.path.join(SRC_DIR, f) for f in os.listdir(SRC_DIR)]
  srcs.append(os.path.join(_HERE, "..", "include", "v4l_hip.h"))
  if not force and os.path.exists(LIB_PATH) and all(
      os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
    return LIB_PATH
  subprocess.run(build_command(), check=True)
  return LIB_PATH


_P = C.c_void_p
_SIGS = {
  "v4l_last_error": (C.c_char_p, []),
  "v4l_version": (C.c_int, []),
  "v4l_abi_sizeof": (C.c_int, [C.c_int]),
  "v4l_net_create": (C.c_int, [C.POINTER(NetCfg), C.POINTER(_P)]),
  "v4l_net_set_categorical": (C.c_int, [_P, C.c_int]),
  "v4l_net_destroy": (None, [_P]),
  "v4l_net_num_params": (C.c_int, [_P]),
  "v4l_net_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  "v4l_net_total_params": (C.c_int64, [_P]),
  "v4l_net_packed_bytes": (C.c_int64, [_P]),
  "v4l_net_table_bytes": (C.c_int64, [_P]),
  "v4l_net_ws_floats": (C.c_int64, [_P, C.c_int, C.c_int]),
  "v4l_net_state_ld": (C.c_int, [_P]),
  "v4l_net_bind": (C.c_int, [_P, C.POINTER(_P), _P, _P, _P]),
  "v4l_net_pack": (C.c_int, [_P, _P]),
  "v4l_ingest": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int64, _P]),
  "v4l_net_forward": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, _P]),
  "v4l_net_out_ptr": (_P, [_P, _P, C.c_int, C.c_int]),
  "v4l_net_dout_ptr": (_P, [_P, _P, C.c_int]),
  "v4l_net_grad_scale": (C.c_float, [_P, C.c_int]),
  "v4l_net_set_grad_scale": (C.c_int, [_P, C.c_float]),
  "v4l_net_backward": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P]),
  "v4l_gauss_head": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
  "v4l_gauss_head_tanh": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
  "v4l_gauss_head_sd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
  "v4l_cat_head": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
  "v4l_cat_sample": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
  "v4l_col0": (C.c_int, [_P, C.c_int, _P, _P]),
  "v4l_gae": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                        _P, _P, _P, _P, _P, _P]),
  "v4l_discount_reward": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_int, _P, _P, _P, _P, _P]),
  "v4l_obs_norm": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, C.c_double, C.c_int, _P, C.c_int64, _P, C.c_int64,
                             _P, C.c_int, C.c_int64, C.c_int64, _P, C.c_int64, _P]),
  "v4l_actor_create": (C.c_int, [_P, _P, C.c_int, C.POINTER(_P)]),
  "v4l_actor_destroy": (None, [_P]),
  "v4l_actor_ws_floats": (C.c_int64, [_P]),
  "v4l_actor_ctl_bytes": (C.c_int64, [_P]),
  "v4l_actor_bind": (C.c_int, [_P, _P, _P, _P]),
  "v4l_actor_seek": (C.c_int, [_P, C.c_int64, _P]),
  "v4l_actor_check": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
  "v4l_actor_step": (C.c_int, [_P] + [_P] * 12 + [C.c_int, C.c_int, _P]),
  "v4l_actor_split_supported": (C.c_int, [_P, C.c_int]),
  "v4l_actor_route": (C.c_char_p, [_P, C.c_int]),
  "v4l_actor_step_split": (C.c_int, [_P] + [_P] * 13 + [C.c_int, _P]),
  "v4l_trainer_create": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
  "v4l_trainer_destroy": (None, [_P]),
  "v4l_trainer_ws_floats": (C.c_int64, [_P, C.c_int]),
  "v4l_trainer_ctl_bytes": (C.c_int64, [_P, C.c_int]),
  "v4l_trainer_bind": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int, _P]),
  "v4l_trainer_begin": (C.c_int, [_P, _P, _P, C.c_double, C.c_double, C.c_int64, C.POINTER(PPOHyper), _P]),
  "v4l_trainer_begin_guarded": (C.c_int, [_P, _P, _P, _P, C.c_double, C.c_double, C.c_int64, C.c_int64, C.POINTER(PPOHyper), _P]),
  "v4l_trainer_steps": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
  "v4l_trainer_kl_stop": (C.c_int, [_P, C.c_double, _P, _P]),
  "v4l_trainer_kl_update_next": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), C.c_int, _P]),
  "v4l_trainer_kl_update_run": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), C.c_int, C.c_int, _P]),
  "v4l_trainer_kl_graph_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  "v4l_trainer_kl_adapt": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P]),
  "v4l_trainer_kl_adapt_update_next": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), C.c_int, _P]),
  "v4l_trainer_kl_adapt_update_run": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), C.c_int, C.c_int, _P]),
  "v4l_trainer_kl_adapt_graph_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  "v4l_trainer_lrs": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
  "v4l_trainer_update_next": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), C.c_int, _P]),
  "v4l_host_cast_rows": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int64, _P, _P, C.c_int, C.c_int]),
  "v4l_host_cast_simd": (C.c_int, []),
  "v4l_actor_step_rows": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int,
                                    C.c_double, _P]),
  "v4l_trainer_update_run": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), C.c_int, C.c_int, _P]),
  "v4l_trainer_critic_grads": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P]),
  "v4l_trainer_critic_step": (C.c_int, [_P, C.POINTER(PPOHyper), _P]),
  "v4l_trainer_actor_grads": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P]),
  "v4l_trainer_actor_step": (C.c_int, [_P, C.POINTER(PPOHyper), _P]),
  "v4l_trainer_stats_cur": (_P, [_P]),
  "v4l_trainer_update": (C.c_int, [_P, C.POINTER(Rollout), _P, C.c_int, C.POINTER(PPOHyper), C.c_double,
                                   C.c_double, C.c_int64, _P, _P]),
  "v4l_trainer_sync_target": (C.c_int, [_P, _P]),
  "v4l_trainer_vmpo_bytes": (C.c_int64, [_P, C.c_int]),
  "v4l_trainer_vmpo_init": (C.c_int, [_P, C.POINTER(VMPOHyper), _P, C.c_int, _P]),
  "v4l_trainer_vmpo_actor_grads": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, _P]),
  "v4l_trainer_vmpo_update_next": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, C.c_int, _P]),
  "v4l_trainer_vmpo_update_run": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, C.c_int, C.c_int, _P]),
  "v4l_trainer_vmpo_graph_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  "v4l_trainer_vmpo_state": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
  "v4l_trainer_vmpo_set_state": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
  "v4l_vmpo_select": (C.c_int, [_P, _P, C.c_int, _P, _P]),
  "v4l_trainer_a2c_critic_grads": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, _P]),
  "v4l_trainer_a2c_actor_grads": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, _P]),
  "v4l_trainer_a2c_update_next": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, C.c_int, _P]),
  "v4l_trainer_a2c_update_run": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, C.c_int, C.c_int, _P]),
  "v4l_trainer_a2c_graph_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  "v4l_trainer_reinforce_actor_grads": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, _P]),
  "v4l_trainer_reinforce_update_next": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, C.c_int, _P]),
  "v4l_trainer_reinforce_update_run": (C.c_int, [_P, C.POINTER(Rollout), C.c_int, C.POINTER(PPOHyper), _P, C.c_int, C.c_int, _P]),
  "v4l_trainer_reinforce_graph_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  "v4l_comm_available": (C.c_int, []),
  "v4l_trainer_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
  "v4l_comm_unique_id": (C.c_int, [C.c_char_p]),
  "v4l_trainer_comm_init": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int]),
  "v4l_trainer_comm_destroy": (C.c_int, [_P]),
  "v4l_sync_grads": (C.c_int, [_P, C.c_int, _P]),
  "v4l_trainer_comm_selftest": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), _P]),
  "v4l_trainer_bucket_tail": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
  "v4l_net_ws_offset": (C.c_int64, [_P, C.c_int, C.c_char_p]),
  "v4l_prof_enable": (C.c_int, [C.c_int]),
  "v4l_prof_collect": (C.c_int64, [C.c_char_p, C.c_int64]),
}

_lib = None


def exported_symbols():
  """Every entry point include/v4l_hip.h declares (checked by the CPU test-suite)."""
  return sorted(_SIGS)


# V4L_* variables that configure a run; every OTHER V4L_* variable is a diagnostic switch that swaps kernels or schedules
# (include/v4l_hip.h lists them) — fine for A/B probes and the cross-check tests, a trap when one is left in a shell by accident
_CONFIG_ENV = {"V4L_COMPUTE", "V4L_GRAPH", "V4L_DP_COMM", "V4L_CAST_THREADS", "V4L_RCCL_LIB", "V4L_TRACE", "V4L_ROCTX", "V4L_LIB"}


def diagnostic_switches():
  """The diagnostic V4L_* switches present in the environment right now (name -> value)."""
  return {k: v for k, v in sorted(os.environ.items()) if k.startswith("V4L_") and k not in _CONFIG_ENV}


def lib():
  global _lib
  if _lib is None:
    active = diagnostic_switches()
    if active:  # said once, when the library is loaded: a stray switch must not change kernels under a user silently
      import warnings
      warnings.warn("vision4leg_amd: diagnostic switches are set and change which kernels / schedules run: %s"
                    % ", ".join("%s=%s" % kv for kv in active.items()), RuntimeWarning, stacklevel=2)
    if not os.path.exists(LIB_PATH):
      raise RuntimeError(
        "vision4leg_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(there is no CPU fallback for the HIP hot path)" % LIB_PATH)
    l = C.CDLL(LIB_PATH)
    rebuild = "rebuild it (python -c 'import __graft_entry__ as g; g.build()')"
    # a stale .so is exactly what the guards below are for, and it lacks the newest symbols: resolve the version / ABI entries
    # first and say "rebuild" instead of dying on a bare AttributeError('undefined symbol') in the binding loop
    try:
      l.v4l_version.restype, l.v4l_version.argtypes = _SIGS["v4l_version"]
      l.v4l_abi_sizeof.restype, l.v4l_abi_sizeof.argtypes = _SIGS["v4l_abi_sizeof"]
    except AttributeError as e:
      raise RuntimeError("vision4leg_amd: %s predates this Python binding (%s) — %s" % (LIB_PATH, e, rebuild)) from None
    # the struct mirrors above must be the structs this library was compiled with (a stale .so next to newer host code reads
    # fields at the wrong offsets otherwise)
    for which, (name, mirror) in ((0, ("v4l_net_cfg", NetCfg)), (1, ("v4l_ppo_hyper", PPOHyper)), (2, ("v4l_rollout", Rollout)),
                                  (4, ("v4l_vmpo_hyper", VMPOHyper))):
      have = l.v4l_abi_sizeof(which)
      if have != C.sizeof(mirror):
        raise RuntimeError("vision4leg_amd: %s was compiled with sizeof(%s) = %d, the Python binding expects %d — %s"
                           % (LIB_PATH, name, have, C.sizeof(mirror), rebuild))
    for name, (res, args) in _SIGS.items():
      try:
        fn = getattr(l, name)
      except AttributeError:
        raise RuntimeError("vision4leg_amd: %s does not export %s — %s" % (LIB_PATH, name, rebuild)) from None
      fn.restype = res
      fn.argtypes = args
    _lib = l
  return _lib


def check(rc, what=""):
  if rc != 0:
    msg = lib().v4l_last_error()
    raise RuntimeError("libv4l_hip %s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))
