"""Which optimiser `PPO(optimizer_class=...)` asks for: the pure, host-only half (torch only, no GPU, no libv4l_hip.so).

The reference builds both optimisers as `optimizer_class(params, lr=..., eps=1e-5)` (torchrl/algo/on_policy/a2c.py:30-40). The HIP
engine runs one kernel for clip + step, so what it needs from the class is a handful of numbers. `resolve` gets them the way the
reference would: it constructs the class once, on a one-element dummy parameter, with the reference's call-time arguments, and reads
`param_groups[0]`. torch's own defaults (AdamW's weight_decay 0.01), a `functools.partial`'s keywords and "the call-time eps=1e-5
wins over a partial's" then come out as torch decides them, not as restated here.
"""
import collections

import torch

CLASSES = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW}
REFUSED_FLAGS = ("amsgrad", "maximize", "differentiable", "capturable")

Resolved = collections.namedtuple("Resolved", "optimizer_class betas eps weight_decay decoupled")


def resolve(optimizer_class=None, optimizer_kwargs=None, lr=3e-4, eps=1e-5):
    """optimizer_class: None / torch.optim.Adam, torch.optim.AdamW, a functools.partial (or any callable) that returns one of them,
    or the strings "Adam" / "AdamW" with a dict `optimizer_kwargs` (JSON configs cannot carry a class).
    -> Resolved(optimizer_class, betas, eps, weight_decay, decoupled). NotImplementedError for another optimiser; ValueError, naming
    the offender, for amsgrad / maximize / differentiable / capturable, several param groups and whatever torch itself refuses
    (a negative weight_decay)."""
    given = optimizer_class
    if given is None:
        given = torch.optim.Adam
    kwargs = {}
    if isinstance(given, str):
        if given not in CLASSES:
            raise NotImplementedError("vision4leg_amd: PPO runs Adam or AdamW on the HIP engine; optimizer_class %r is neither "
                                      "(strings: %s)" % (given, ", ".join(sorted(CLASSES))))
        given = CLASSES[given]
        kwargs = dict(optimizer_kwargs or {})
    elif optimizer_kwargs:
        raise ValueError("vision4leg_amd: optimizer_kwargs goes with optimizer_class given as a string (\"Adam\" / \"AdamW\"); "
                         "with a class, use functools.partial")
    if not callable(given):
        raise NotImplementedError("vision4leg_amd: optimizer_class %r is not an optimiser class" % (given,))
    for key in ("lr", "eps"):
        if key in kwargs:
            raise ValueError("vision4leg_amd: optimizer_kwargs[%r]: PPO passes lr (plr / vlr) and eps=1e-5 itself, as the "
                             "reference does" % key)
    inner = given
    while hasattr(inner, "func"):  # functools.partial (of a partial)
        inner = inner.func
    name = getattr(inner, "__qualname__", None) or repr(inner)
    if isinstance(inner, type) and issubclass(inner, torch.optim.Optimizer) and inner not in (torch.optim.Adam, torch.optim.AdamW):
        # (before the call: SGD, for one, takes no eps and would die on the reference's own call with a TypeError)
        raise NotImplementedError("vision4leg_amd: PPO runs Adam or AdamW on the HIP engine; optimizer_class is %s" % name)
    try:
        # eps=None: the reference's Reinforce call, `optimizer_class(params, lr=...)` (reinforce.py:26-29): torch's (or a
        # partial's) own eps
        call = {"lr": lr} if eps is None else {"lr": lr, "eps": eps}
        opt = given([torch.nn.Parameter(torch.zeros(1))], **call, **kwargs)
    except TypeError as e:
        raise ValueError("vision4leg_amd: optimizer_class %s cannot be built as the reference builds it, "
                         "optimizer_class(params, lr=..., eps=1e-5): %s" % (name, e)) from None
    if type(opt) not in (torch.optim.Adam, torch.optim.AdamW):
        raise NotImplementedError("vision4leg_amd: PPO runs Adam or AdamW on the HIP engine; optimizer_class gave %s.%s"
                                  % (type(opt).__module__, type(opt).__qualname__))
    if len(opt.param_groups) != 1:
        raise ValueError("vision4leg_amd: the HIP engine runs one param group per optimiser, optimizer_class made %d"
                         % len(opt.param_groups))
    g = opt.param_groups[0]
    for key in REFUSED_FLAGS:
        if g.get(key):
            raise ValueError("vision4leg_amd: the HIP engine runs %s without %s=True" % (type(opt).__name__, key))
    if isinstance(g["lr"], torch.Tensor) or isinstance(g["weight_decay"], torch.Tensor):
        raise ValueError("vision4leg_amd: tensor-valued lr / weight_decay are not supported")
    wd = float(g["weight_decay"])
    if not (wd >= 0.0 and wd != float("inf")):
        raise ValueError("vision4leg_amd: weight_decay must be finite and >= 0 (got %r)" % (g["weight_decay"],))
    b1, b2 = g["betas"]
    return Resolved(type(opt), (float(b1), float(b2)), float(g["eps"]), g["weight_decay"], bool(g.get("decoupled_weight_decay", False)))


def group_mismatch(group, betas, eps, weight_decay, decoupled):
    """A loaded param group against what the engine runs -> None, or a message that names both sides. Keys the file does not hold
    are not compared, except the decoupled flag: a group without it is L2 decay (Adam.__setstate__'s default)."""
    if "betas" in group and tuple(float(b) for b in group["betas"]) != tuple(float(b) for b in betas) \
            or "eps" in group and float(group["eps"]) != float(eps):
        return "the optimiser state was written with betas %s / eps %s, the HIP engine runs %s / %s" \
               % (group.get("betas"), group.get("eps"), betas, eps)
    wd_file = float(group.get("weight_decay", 0) or 0)
    dec_file = bool(group.get("decoupled_weight_decay", False))
    # without decay the two classes are one optimiser: the flag only matters next to a decay
    if wd_file != float(weight_decay) or (wd_file != 0 and dec_file != bool(decoupled)):
        return "the optimiser state was written with weight_decay %r (%s), the HIP engine runs weight_decay %r (%s)" \
               % (group.get("weight_decay", 0), "decoupled, AdamW" if dec_file else "coupled L2, Adam",
                  weight_decay, "decoupled, AdamW" if decoupled else "coupled L2, Adam")
    return None
