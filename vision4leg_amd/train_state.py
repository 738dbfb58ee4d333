"""Resumable training state: the pure, host-only half.

The HIP engine keeps each optimiser's Adam moments in two flat fp32 device buffers in plan order (`HipNet.param_names /
param_shapes / grad_offsets`, the layout `HipNet.grad_view` reads) and ONE step count per optimiser. `torch.optim.Adam` keeps
`{"step", "exp_avg", "exp_avg_sq"}` per parameter, keyed by the position in `module.parameters()`. The functions here translate
between the two, both ways, so that a run can be continued on either side (`torch.optim.Adam(net.parameters(), lr, eps=1e-5)`,
torchrl/algo/a2c.py:24-27; with weight decay `Adam(weight_decay=...)` or `AdamW`), and pack / unpack the parts of `train_state_{epoch}.pth` that are not tensors already.

Nothing here touches the GPU or libv4l_hip.so: torch and numpy only (tests/test_resume_cpu.py).
"""
import os
import re

import numpy as np
import torch

FORMAT_VERSION = 1
FILE = "train_state_{}.pth"


# ---- parameter position <-> flat slice -------------------------------------------------------------------------------------
def param_slices(plan, module):
    """-> [(name, shape, offset, numel)] in `module.parameters()` order. `plan`: anything with `param_names`, `param_shapes` and
    `grad_offsets` (a HipNet). Raises, naming the parameter, for one the plan does not cover, for a shape the plan does not
    expect, and for a plan entry that `parameters()` never reaches (its moments would be lost)."""
    where = {n: i for i, n in enumerate(plan.param_names)}
    out, seen = [], set()
    for name, p in module.named_parameters():
        i = where.get(name)
        if i is None:
            raise KeyError("vision4leg_amd: parameter %r of the module is not covered by the HIP plan" % name)
        shp = tuple(int(d) for d in plan.param_shapes[i])
        if tuple(p.shape) != shp:
            raise ValueError("vision4leg_amd: parameter %s has shape %s, the HIP plan expects %s" % (name, tuple(p.shape), shp))
        out.append((name, shp, int(plan.grad_offsets[i]), int(np.prod(shp, dtype=np.int64))))
        seen.add(name)
    for name in plan.param_names:
        if name not in seen:
            raise KeyError("vision4leg_amd: plan parameter %r is not among the module's parameters()" % name)
    return out


def flat_size(slices):
    return max((off + n for _, _, off, n in slices), default=0)


def export_adam(slices, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-5, weight_decay=0, decoupled=False):
    """Flat moment buffers + one step count -> what `torch.optim.Adam(...).state_dict()` returns after `step` steps: CPU fp32
    copies in the parameters' shapes, `step` a float32 scalar tensor per parameter; an empty `state` before the first step.
    weight_decay goes into the group as given; `decoupled_weight_decay: True` is written only for a decoupled (AdamW) optimiser —
    a real AdamW that loads a group without the key falls back to L2 decay (Adam.__setstate__), and an L2 / no-decay group stays
    the six keys it always was."""
    state = {}
    if step > 0:
        m, v = exp_avg.detach().to("cpu", torch.float32), exp_avg_sq.detach().to("cpu", torch.float32)
        for i, (_, shp, off, n) in enumerate(slices):
            state[i] = {"step": torch.tensor(float(step), dtype=torch.float32),
                        "exp_avg": m[off:off + n].reshape(shp).clone(), "exp_avg_sq": v[off:off + n].reshape(shp).clone()}
    group = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "weight_decay": weight_decay, "amsgrad": False,
             "params": list(range(len(slices)))}
    if decoupled:
        group["decoupled_weight_decay"] = True
    return {"state": state, "param_groups": [group]}


def _step_of(value, name):
    s = float(value)  # a tensor (current torch) or a plain number (older files)
    if s != int(s) or s < 0:
        raise ValueError("vision4leg_amd: Adam step %r of parameter %s is not a count" % (s, name))
    return int(s)


def import_adam(slices, sd, total=None):
    """The inverse of export_adam, for a dict written by it or by a real `torch.optim.Adam` over the same module:
    -> (exp_avg [total] fp32, exp_avg_sq [total] fp32, step, param_group). An empty `state` gives zero moments and step 0.
    Raises, naming the parameter, for a parameter without state next to ones that have it, for a mis-shaped moment, and for
    per-parameter step counts that disagree (the engine keeps one count per optimiser)."""
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError("vision4leg_amd: expected one Adam param_group, got %d" % len(groups))
    group = groups[0]
    ids = list(group["params"])
    if len(ids) != len(slices):
        raise ValueError("vision4leg_amd: the optimiser state covers %d parameters, the module has %d" % (len(ids), len(slices)))
    for key in ("amsgrad", "maximize"):  # (weight decay is the caller's to compare with what it runs: the group is returned)
        if group.get(key):
            raise ValueError("vision4leg_amd: the HIP engine runs Adam / AdamW without %s" % key)
    total = flat_size(slices) if total is None else int(total)
    m, v = torch.zeros(total, dtype=torch.float32), torch.zeros(total, dtype=torch.float32)
    state, step = sd["state"], None
    if len(state) == 0:
        return m, v, 0, group
    for pid, (name, shp, off, n) in zip(ids, slices):
        st = state.get(pid)
        if st is None:
            raise KeyError("vision4leg_amd: the optimiser state has no entry for parameter %s" % name)
        for key, flat in (("exp_avg", m), ("exp_avg_sq", v)):
            t = st[key]
            if tuple(t.shape) != shp:
                raise ValueError("vision4leg_amd: %s of parameter %s has shape %s, expected %s" % (key, name, tuple(t.shape), shp))
            flat[off:off + n].copy_(t.detach().to("cpu", torch.float32).reshape(-1))
        s = _step_of(st["step"], name)
        if step is None:
            step, first = s, name
        elif s != step:
            raise ValueError("vision4leg_amd: Adam step counts disagree inside one optimiser: %s has %d, %s has %d "
                             "(the HIP engine keeps one count per optimiser)" % (name, s, first, step))
    return m, v, step, group


# ---- the parts of the file that are not tensors already --------------------------------------------------------------------
def pack_numpy_rng(state=None):
    """numpy's global MT19937 state as {str, tensor, numbers}: what torch.load(weights_only=True) reads back."""
    kind, key, pos, has_gauss, cached = np.random.get_state() if state is None else state
    return {"kind": str(kind), "key": torch.from_numpy(np.asarray(key, dtype=np.int64).copy()), "pos": int(pos),
            "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}


def unpack_numpy_rng(d):
    """-> the tuple np.random.set_state takes."""
    return (str(d["kind"]), d["key"].numpy().astype(np.uint32), int(d["pos"]), int(d["has_gauss"]), float(d["cached_gaussian"]))


def plain_rewards(values):
    """A reward deque as plain numbers / nested lists. The entries keep their shapes — the collector appends [1] arrays for eval
    episodes and scalars for training episodes, and np.mean over a deque needs old and new entries to agree."""
    return [np.asarray(v, dtype=np.float64).tolist() for v in values]


def restore_rewards(values):
    """The inverse of plain_rewards: float64 scalars / arrays in the saved shapes."""
    return [np.float64(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64) for v in values]


def optional_tensor(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64, copy=True))


def path(prefix, epoch):
    return os.path.join(prefix, FILE.format(epoch))


def newest(directory):
    """-> the largest epoch number N for which `directory/train_state_N.pth` exists (tags such as "finish" or "best" are not
    numbers and are never picked), or None."""
    best = None
    for f in os.listdir(directory):
        m = re.fullmatch(r"train_state_(\d+)\.pth", f)
        if m and (best is None or int(m.group(1)) > best):
            best = int(m.group(1))
    return best


def load(prefix, epoch):
    """Read train_state_{epoch}.pth with the restricted unpickler and check its format version."""
    st = torch.load(path(prefix, epoch), map_location="cpu", weights_only=True)
    if st.get("format_version") != FORMAT_VERSION:
        raise RuntimeError("vision4leg_amd: %s has format version %r, this build reads %d"
                           % (path(prefix, epoch), st.get("format_version"), FORMAT_VERSION))
    return st
