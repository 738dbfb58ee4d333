"""Overlay of the MI355X hot path onto the reference's in-tree `torchrl` package.

`install()` imports the reference package (it must be importable: /path/to/vision4leg on sys.path) and rebinds ONLY the
hot-path names — the classes SURVEY.md §8(b) lists — on the reference's own modules. Everything else the starters import
(`torchrl.algo.VMPO`, `torchrl.utils.Logger`, `torchrl.env.get_vec_env`, the other policies / algorithms / collectors)
stays the reference's, so `starter/ppo_*.py` runs unchanged:

    import vision4leg_amd.overlay as overlay
    overlay.install()                 # pf.explore / vf / PPO.update / GAE on the HIP engine, reference collector
    overlay.install(fast_path=True)   # + fused rollout step, HBM-resident replay buffer, pinned observation upload
    overlay.install(vmpo=True)        # + `torchrl.algo.VMPO` on the HIP engine (opt-in: the default leaves it the reference's)
    overlay.install(a2c=True)         # + `torchrl.algo.A2C` on the HIP engine, state-MLP nets only (opt-in, like vmpo)
    overlay.install(reinforce=True)   # + `torchrl.algo.Reinforce` on the HIP engine, `networks.ZeroNet` -> this package's (opt-in)
    overlay.install(state_std=True)   # + `torchrl.policies.GaussianContPolicy` (log-std from the head) on the HIP engine (opt-in)
    overlay.install(discrete=True)    # + `torchrl.policies.CategoricalDisPolicy` (discrete actions, under A2C / Reinforce) and
                                      #   `torchrl.algo.PPODiscrete`, its PPO learner, a name the reference does not have (opt-in)

Rebinding is by name on every already-imported `torchrl.<pkg>` module that defines the name (the package and the
sub-module that holds the class: `from torchrl.algo import PPO`, `from torchrl.algo.on_policy.ppo import PPO` and
`torchrl.networks.nets.LocoTransformer` all resolve to the HIP class afterwards).
"""
import importlib
import sys

# reference package -> hot-path names taken from the same-named shell package
HOT_NAMES = {
    "networks": ["MLPBase", "NatureEncoder", "NatureFuseEncoder", "LocoTransformerEncoder", "TransformerEncoder",
                 "Net", "ImpalaEncoderProjNet", "LocoTransformer", "NatureEncoderProjNet", "Transformer"],
    "policies": ["GaussianContPolicyBasicBias", "GaussianContPolicyImpalaEncoderProj",
                 "GaussianContPolicyLocoTransformer", "GaussianContPolicyNatureEncoderProj",
                 "GaussianContPolicyTransformer"],
    "algo": ["PPO"],
    "replay_buffers": ["OnPolicyReplayBuffer"],
}
# names the reference does not have (the MI355X-native additions); attached to the package for `from torchrl.x import y`
NEW_NAMES = {
    "policies": ["RolloutActor"],
    "replay_buffers": ["DeviceOnPolicyReplayBuffer"],
}
# fast_path=True: the starters' `OnPolicyReplayBuffer(...)` / `VecOnPolicyCollector(...)` construct these instead
FAST_NAMES = {
    "replay_buffers": {"OnPolicyReplayBuffer": "DeviceOnPolicyReplayBuffer"},
    "collector": {"VecOnPolicyCollector": "VecOnPolicyCollector"},
}

# vmpo=True: the second on-policy learner of the starters' `from torchrl.algo import PPO, VMPO`
VMPO_NAMES = {
    "algo": ["VMPO"],
}

# a2c=True: the plain actor-critic both learners derive from (`from torchrl.algo import A2C`)
A2C_NAMES = {
    "algo": ["A2C"],
}

# reinforce=True: the critic-free learner (`from torchrl.algo import Reinforce`). The reference's Reinforce imports ZeroNet for
# its vacant critic; a starter that hands `networks.ZeroNet()` to the fast-path collector gets this package's class, which the
# collector and algo.Reinforce turn into networks.zero_critic(pf) (rebound silently: the report names the learner only)
REINFORCE_NAMES = {
    "algo": ["Reinforce"],
}
REINFORCE_SILENT = {
    "networks": ["ZeroNet"],
}

# state_std=True: the Gaussian policy with a state-dependent log-std head (continuous_policy.py:222-236), state-MLP nets under PPO
STATE_STD_NAMES = {
    "policies": ["GaussianContPolicy"],
}

# discrete=True: the categorical policy over K discrete actions (discrete_policies.py:127-172), state-MLP nets under A2C / Reinforce
DISCRETE_NAMES = {
    "policies": ["CategoricalDisPolicy"],
}
# ... and its PPO learner: a name the reference does not have, so nothing is rebound; attached to the package for
# `from torchrl.algo import PPODiscrete` (silently: the report names what was replaced)
DISCRETE_NEW = {
    "algo": ["PPODiscrete"],
}

_installed = {}


def _rebind(ref_pkg_name, name, obj, always_on_package=False):
    """Set `name` on torchrl.<pkg> and on each imported sub-module of it that already defines `name`."""
    hits = []
    prefix = ref_pkg_name + "."
    for modname, mod in list(sys.modules.items()):
        if mod is None or not (modname == ref_pkg_name or modname.startswith(prefix)):
            continue
        if name in getattr(mod, "__dict__", {}) or (always_on_package and modname == ref_pkg_name):
            _installed.setdefault((modname, name), mod.__dict__.get(name))
            setattr(mod, name, obj)
            hits.append(modname)
    return hits


def install(fast_path=False, reference_package="torchrl", vmpo=False, a2c=False, state_std=False, reinforce=False, discrete=False):
    """Rebind the hot-path classes on the reference's `torchrl`. Returns {"pkg.name": [modules patched]}.
    vmpo=True also rebinds `torchrl.algo.VMPO` (vision4leg_amd.torchrl.algo.VMPO); without it VMPO stays the reference's.
    a2c=True also rebinds `torchrl.algo.A2C` (and nothing else); without it A2C stays the reference's.
    reinforce=True also rebinds `torchrl.algo.Reinforce` and `torchrl.networks.ZeroNet` (the report gains "algo.Reinforce" only);
    without it both stay the reference's.
    state_std=True also rebinds `torchrl.policies.GaussianContPolicy` (and nothing else); without it that class stays the reference's.
    discrete=True also rebinds `torchrl.policies.CategoricalDisPolicy` and puts `PPODiscrete` on `torchrl.algo` (a new name: nothing
    is rebound, the report does not list it); without it that class stays the reference's and `torchrl.algo` has no such name."""
    ref = importlib.import_module(reference_package)
    if getattr(ref, "__v4l_shell__", False):
        raise RuntimeError("vision4leg_amd.overlay: `%s` resolves to the HIP shell itself; put the reference "
                           "checkout first on sys.path" % reference_package)
    report = {}
    for pkg, names in HOT_NAMES.items():
        ref_name = "%s.%s" % (reference_package, pkg)
        importlib.import_module(ref_name)
        shell = importlib.import_module("vision4leg_amd.torchrl." + pkg)
        for name in names:
            hits = _rebind(ref_name, name, getattr(shell, name))
            if not hits:
                raise RuntimeError("vision4leg_amd.overlay: the reference has no %s.%s to replace" % (ref_name, name))
            report["%s.%s" % (pkg, name)] = hits
    for pkg, names in NEW_NAMES.items():
        shell = importlib.import_module("vision4leg_amd.torchrl." + pkg)
        for name in names:
            report["%s.%s" % (pkg, name)] = _rebind("%s.%s" % (reference_package, pkg), name, getattr(shell, name), True)
    if fast_path:
        for pkg, names in FAST_NAMES.items():
            ref_name = "%s.%s" % (reference_package, pkg)
            importlib.import_module(ref_name)
            shell = importlib.import_module("vision4leg_amd.torchrl." + pkg)
            for name, shell_name in names.items():
                report["%s.%s" % (pkg, name)] = _rebind(ref_name, name, getattr(shell, shell_name))
    if reinforce:
        for pkg, names in REINFORCE_SILENT.items():
            ref_name = "%s.%s" % (reference_package, pkg)
            shell = importlib.import_module("vision4leg_amd.torchrl." + pkg)
            for name in names:
                if not _rebind(ref_name, name, getattr(shell, name)):
                    raise RuntimeError("vision4leg_amd.overlay: the reference has no %s.%s to replace" % (ref_name, name))
    if discrete:
        for pkg, names in DISCRETE_NEW.items():
            ref_name = "%s.%s" % (reference_package, pkg)
            importlib.import_module(ref_name)
            shell = importlib.import_module("vision4leg_amd.torchrl." + pkg)
            for name in names:
                _rebind(ref_name, name, getattr(shell, name), True)
    for wanted, table in ((vmpo, VMPO_NAMES), (a2c, A2C_NAMES), (state_std, STATE_STD_NAMES), (reinforce, REINFORCE_NAMES),
                          (discrete, DISCRETE_NAMES)):
        if not wanted:
            continue
        for pkg, names in table.items():
            ref_name = "%s.%s" % (reference_package, pkg)
            shell = importlib.import_module("vision4leg_amd.torchrl." + pkg)
            for name in names:
                hits = _rebind(ref_name, name, getattr(shell, name))
                if not hits:
                    raise RuntimeError("vision4leg_amd.overlay: the reference has no %s.%s to replace" % (ref_name, name))
                report["%s.%s" % (pkg, name)] = hits
    return report


def uninstall():
    """Put the reference's own objects back (tests)."""
    for (modname, name), old in list(_installed.items()):
        mod = sys.modules.get(modname)
        if mod is not None:
            if old is None:
                mod.__dict__.pop(name, None)
            else:
                setattr(mod, name, old)
    _installed.clear()
