"""Resumable training state without a GPU: the mapping between the engine's flat Adam moment buffers and
torch.optim.Adam's per-parameter state, in both directions against a real torch.optim.Adam, and the parts of
train_state_{epoch}.pth that have to survive torch.load(weights_only=True). The device side is tests/test_gpu_resume.py."""
import copy
import inspect

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repository root on sys.path)


def _ts():
    from vision4leg_amd import train_state
    return train_state


class _Net(torch.nn.Module):
    """Small module whose parameters() order differs from the plan's order below."""

    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.Linear(5, 4))
        self.head = torch.nn.Linear(4, 2)
        self.logstd = torch.nn.Parameter(torch.zeros(1, 2))


class _Plan:
    """Stand-in for HipNet's plan: names / shapes / offsets into the flat buffers, in an order of its own and with an unused gap
    between two segments (offsets need not be dense)."""

    def __init__(self, module, order=None, gap=8):
        named = dict(module.named_parameters())
        names = list(named) if order is None else order
        self.param_names, self.param_shapes, self.grad_offsets = [], [], []
        off = 0
        for k, name in enumerate(names):
            self.param_names.append(name)
            self.param_shapes.append(tuple(named[name].shape))
            self.grad_offsets.append(off)
            off += named[name].numel() + (gap if k == 1 else 0)
        self.total_params = off


def _setup(seed=0):
    torch.manual_seed(seed)
    net = _Net()
    names = [n for n, _ in net.named_parameters()]
    plan = _Plan(net, order=names[::-1])
    return net, plan


def _covered(plan):
    mask = torch.zeros(plan.total_params, dtype=torch.bool)
    for shp, off in zip(plan.param_shapes, plan.grad_offsets):
        mask[off:off + int(np.prod(shp))] = True
    return mask


def test_flat_to_state_dict_to_flat_is_the_identity():
    ts = _ts()
    net, plan = _setup()
    slices = ts.param_slices(plan, net)
    assert [s[0] for s in slices] == [n for n, _ in net.named_parameters()]
    mask = _covered(plan)
    assert int((~mask).sum()) == 8  # the gap
    m = torch.randn(plan.total_params) * mask
    v = torch.rand(plan.total_params) * mask
    sd = ts.export_adam(slices, m, v, 7, 2.5e-4)
    # every exp_avg[i] is the flat slice at that parameter's offset, reshaped — the layout HipNet.grad_view reads
    for i, (name, p) in enumerate(net.named_parameters()):
        j = plan.param_names.index(name)
        off, shp = plan.grad_offsets[j], plan.param_shapes[j]
        st = sd["state"][i]
        assert st["exp_avg"].shape == p.shape and st["exp_avg"].dtype == torch.float32 and st["exp_avg"].device.type == "cpu"
        assert torch.equal(st["exp_avg"], m[off:off + p.numel()].view(shp)), name
        assert torch.equal(st["exp_avg_sq"], v[off:off + p.numel()].view(shp)), name
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 7.0
    g, = sd["param_groups"]
    assert g == {"lr": 2.5e-4, "betas": (0.9, 0.999), "eps": 1e-5, "weight_decay": 0, "amsgrad": False,
                 "params": list(range(len(slices)))}
    m2, v2, step, group = ts.import_adam(slices, sd, plan.total_params)
    assert torch.equal(m2, m) and torch.equal(v2, v) and step == 7 and group["lr"] == 2.5e-4
    # copies, not views of the flat buffers
    sd["state"][0]["exp_avg"].add_(1.0)
    assert torch.equal(ts.import_adam(slices, ts.export_adam(slices, m, v, 7, 1e-4), plan.total_params)[0], m)


def test_before_the_first_step_the_state_is_empty_and_loads_as_zero():
    ts = _ts()
    net, plan = _setup()
    slices = ts.param_slices(plan, net)
    sd = ts.export_adam(slices, torch.zeros(plan.total_params), torch.zeros(plan.total_params), 0, 3e-4)
    fresh = torch.optim.Adam(net.parameters(), lr=3e-4, eps=1e-5).state_dict()
    assert sd["state"] == {} == fresh["state"]
    assert sd["param_groups"][0]["params"] == fresh["param_groups"][0]["params"]
    m, v, step, _ = ts.import_adam(slices, fresh, plan.total_params)
    assert step == 0 and not m.any() and not v.any() and m.numel() == plan.total_params


def _stepped_adam(net, steps=2, seed=1):
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-5)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt


def test_a_real_torch_adam_state_goes_into_the_flat_buffers():
    ts = _ts()
    net, plan = _setup()
    opt = _stepped_adam(net)
    slices = ts.param_slices(plan, net)
    m, v, step, group = ts.import_adam(slices, opt.state_dict(), plan.total_params)
    assert step == 2 and group["lr"] == 1e-3
    # the concatenation of torch's own moments in PLAN order (the gap stays zero)
    named = dict(net.named_parameters())
    want_m, want_v = torch.zeros(plan.total_params), torch.zeros(plan.total_params)
    for name, off in zip(plan.param_names, plan.grad_offsets):
        st = opt.state[named[name]]
        want_m[off:off + named[name].numel()] = st["exp_avg"].reshape(-1)
        want_v[off:off + named[name].numel()] = st["exp_avg_sq"].reshape(-1)
    assert torch.equal(m, want_m) and torch.equal(v, want_v)
    assert m.abs().sum() > 0 and v.sum() > 0


def test_the_export_loads_into_a_real_torch_adam():
    ts = _ts()
    net, plan = _setup()
    opt = _stepped_adam(net)
    slices = ts.param_slices(plan, net)
    m, v, step, group = ts.import_adam(slices, opt.state_dict(), plan.total_params)
    sd = ts.export_adam(slices, m, v, step, group["lr"])
    other = torch.optim.Adam(copy.deepcopy(net).parameters(), lr=5e-2, eps=1e-5)
    other.load_state_dict(sd)  # accepted without error
    got, want = other.state_dict(), opt.state_dict()
    assert sorted(got["state"]) == sorted(want["state"]) == list(range(len(slices)))
    for i in want["state"]:
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(got["state"][i][key], want["state"][i][key]), (i, key)
    assert got["param_groups"][0]["lr"] == 1e-3 and got["param_groups"][0]["eps"] == 1e-5
    # ... and that optimiser can go on stepping from there exactly like the original
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(p.shape, generator=gen) for p in net.parameters()]
    twin = list(other.param_groups[0]["params"])
    for p, q, g in zip(net.parameters(), twin, grads):
        p.grad, q.grad = g.clone(), g.clone()
    opt.step(); other.step()
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), twin))


def test_disagreeing_step_counts_raise():
    ts = _ts()
    net, plan = _setup()
    slices = ts.param_slices(plan, net)
    sd = _stepped_adam(net).state_dict()
    sd["state"][2]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match=r"step counts disagree.*%s" % slices[2][0].replace(".", r"\.")):
        ts.import_adam(slices, sd, plan.total_params)


def test_missing_and_misshaped_parameters_raise_and_are_named():
    ts = _ts()
    net, plan = _setup()
    slices = ts.param_slices(plan, net)
    # a parameter of parameters() the plan does not cover
    short = _Plan(net, order=[n for n, _ in net.named_parameters() if n != "head.bias"])
    with pytest.raises(KeyError, match="head.bias"):
        ts.param_slices(short, net)
    # a shape the plan does not expect
    wrong = _Plan(net)
    wrong.param_shapes[wrong.param_names.index("encoder.1.weight")] = (5, 4)
    with pytest.raises(ValueError, match=r"encoder\.1\.weight.*\(4, 5\).*\(5, 4\)"):
        ts.param_slices(wrong, net)
    # a plan entry the module's parameters() never reach
    extra = _Plan(net)
    extra.param_names.append("ghost.weight"); extra.param_shapes.append((3,)); extra.grad_offsets.append(extra.total_params)
    with pytest.raises(KeyError, match="ghost.weight"):
        ts.param_slices(extra, net)
    # an optimiser state without an entry for one parameter / with a moment of another shape
    sd = _stepped_adam(net).state_dict()
    gone = copy.deepcopy(sd)
    del gone["state"][1]
    with pytest.raises(KeyError, match=slices[1][0].replace(".", r"\.")):
        ts.import_adam(slices, gone, plan.total_params)
    bent = copy.deepcopy(sd)
    bent["state"][3]["exp_avg_sq"] = torch.zeros(7)
    with pytest.raises(ValueError, match=r"exp_avg_sq of parameter %s" % slices[3][0].replace(".", r"\.")):
        ts.import_adam(slices, bent, plan.total_params)
    # a state for another number of parameters
    fewer = copy.deepcopy(sd)
    fewer["param_groups"][0]["params"] = fewer["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError, match="covers"):
        ts.import_adam(slices, fewer, plan.total_params)


def test_train_state_file_round_trips_through_the_restricted_unpickler(tmp_path):
    ts = _ts()
    net, plan = _setup()
    slices = ts.param_slices(plan, net)
    opt = _stepped_adam(net)
    m, v, step, group = ts.import_adam(slices, opt.state_dict(), plan.total_params)
    np.random.seed(1234)
    np.random.permutation(50); np.random.randn(3)  # somewhere inside the stream, with a cached gaussian
    torch.manual_seed(77)
    state = {
        "format_version": ts.FORMAT_VERSION,
        "pf_optimizer": ts.export_adam(slices, m, v, step, group["lr"]),
        "vf_optimizer": ts.export_adam(slices, m, v, 0, 3e-4),
        "epoch": 2, "total_frames": 49152, "training_update_num": 144, "best_eval": None,
        "episode_rewards": ts.plain_rewards([np.float64(1.5), np.array([2.5]), 3.0]),
        "training_episode_rewards": [],
        "skipped_steps": {"pf": 1, "vf": 0}, "f16_saturated": 0.0,
        "compute": "f16", "net_kinds": {"pf": 2, "vf": 2},
        "rng": {"numpy": ts.pack_numpy_rng(), "torch_cpu": torch.get_rng_state(), "torch_cuda": torch.zeros(16, dtype=torch.uint8)},
        "collector": {"current_step": ts.optional_tensor(np.arange(4.0).reshape(4, 1)), "train_rew": ts.optional_tensor(None)},
    }
    want_perm, want_torch = np.random.permutation(20), torch.rand(5)
    want_gauss = np.random.randn(2)
    torch.save(state, ts.path(str(tmp_path), 2))
    back = ts.load(str(tmp_path), 2)  # torch.load(..., weights_only=True)
    assert back["episode_rewards"] == [1.5, [2.5], 3.0] and back["best_eval"] is None and back["skipped_steps"] == {"pf": 1, "vf": 0}
    assert back["collector"]["train_rew"] is None and back["collector"]["current_step"].shape == (4, 1)
    assert back["vf_optimizer"]["state"] == {}
    m2, v2, step2, _ = ts.import_adam(slices, back["pf_optimizer"], plan.total_params)
    assert torch.equal(m2, m) and torch.equal(v2, v) and step2 == 2
    restored = ts.restore_rewards(back["episode_rewards"]) + [np.array([4.5])]  # old and new [1] entries average together
    assert [np.shape(r) for r in restored] == [(), (1,), (), (1,)]
    assert np.mean(restored[1::2]) == 3.5 and np.mean(restored[0::2]) == 2.25
    # the RNG streams continue where they were
    np.random.seed(0); torch.manual_seed(0)
    np.random.set_state(ts.unpack_numpy_rng(back["rng"]["numpy"]))
    torch.set_rng_state(back["rng"]["torch_cpu"])
    assert np.array_equal(np.random.permutation(20), want_perm) and torch.equal(torch.rand(5), want_torch)
    assert np.array_equal(np.random.randn(2), want_gauss)
    # another format version is refused
    state["format_version"] = ts.FORMAT_VERSION + 1
    torch.save(state, ts.path(str(tmp_path), 3))
    with pytest.raises(RuntimeError, match="format version"):
        ts.load(str(tmp_path), 3)


def test_newest_picks_the_largest_epoch_number_and_no_tag(tmp_path):
    ts = _ts()
    assert ts.newest(str(tmp_path)) is None
    for tag in ("0", "2", "10", "finish", "best"):
        (tmp_path / ("train_state_%s.pth" % tag)).write_bytes(b"")
    (tmp_path / "model_pf_99.pth").write_bytes(b"")
    assert ts.newest(str(tmp_path)) == 10


def test_ppo_takes_the_two_switches_as_keywords_and_keeps_the_epoch_hook():
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    sig = inspect.signature(ppo.PPO.__init__)
    assert sig.parameters["save_train_state"].default is False and sig.parameters["resume"].default is None
    for name in ("save_checkpoint", "load_checkpoint", "train_state"):
        assert callable(getattr(ppo.PPO, name))
    calls = []
    first = ppo._StartEpoch(3, lambda: calls.append(1))
    assert first == 3 and list(range(first, 5)) == [3, 4] and first + 1 == 4
    first()
    assert calls == [1]


@pytest.mark.parametrize("name", sorted(util.CASES))
def test_every_net_geometry_maps_onto_its_plan(name):
    """The real plans (libv4l_hip.so, no GPU needed to build one): every parameter of parameters() has a slice, the slices do not
    overlap and together they are the whole flat buffer — for both nets, shared encoder included."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    ts = _ts()
    torch.manual_seed(0)
    for net in util.build_nets(networks, policies, util.CASES[name]):
        slices = ts.param_slices(net.hip, net)
        assert [s[0] for s in slices] == [n for n, _ in net.named_parameters()]
        hit = torch.zeros(net.hip.total_params, dtype=torch.int32)
        for _, _, off, n in slices:
            hit[off:off + n] += 1
        assert bool((hit == 1).all()), name


class _Trainer:
    """Host stand-in with HipTrainer's buffer-level pair (adam_state / load_adam_state) over CPU tensors."""

    def __init__(self, pf_plan, vf_plan):
        self.pf, self.vf = pf_plan, vf_plan
        self.m_pf, self.v_pf = torch.zeros(pf_plan.total_params), torch.zeros(pf_plan.total_params)
        self.m_vf, self.v_vf = torch.zeros(vf_plan.total_params), torch.zeros(vf_plan.total_params)
        self.steps, self.step = (0, 0), 0

    def adam_state(self):
        return self.m_pf, self.v_pf, self.m_vf, self.v_vf, self.steps

    def load_adam_state(self, m_pf=None, v_pf=None, m_vf=None, v_vf=None, steps=(None, None), updates=None):
        for dst, src in ((self.m_pf, m_pf), (self.v_pf, v_pf), (self.m_vf, m_vf), (self.v_vf, v_vf)):
            if src is not None:
                dst.copy_(src)
        self.steps = tuple(c if s is None else s for s, c in zip(steps, self.steps))


def test_the_optimiser_facades_load_one_side_each_in_place():
    from vision4leg_amd.torchrl.algo.on_policy.ppo import _HipAdam
    pf, plan_pf = _setup(0)
    vf, plan_vf = _setup(1)
    tr = _Trainer(plan_pf, plan_vf)
    opt_pf, opt_vf = _HipAdam(pf.parameters(), lr=3e-4), _HipAdam(vf.parameters(), lr=1e-4)
    with pytest.raises(RuntimeError, match="not attached"):
        opt_pf.state_dict()
    opt_pf.attach(tr, 0, pf)
    opt_vf.attach(tr, 1, vf)
    assert opt_pf.state_dict()["state"] == {} and opt_pf.state_dict()["param_groups"][0]["lr"] == 3e-4
    addresses = [b.data_ptr() for b in (tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf)]
    ref_pf, ref_vf = _stepped_adam(pf, steps=4, seed=3), _stepped_adam(vf, steps=5, seed=4)
    opt_pf.load_state_dict(ref_pf.state_dict())
    assert tr.steps == (4, 0) and not tr.m_vf.any() and opt_pf.lr == 1e-3 and opt_vf.lr == 1e-4
    opt_vf.load_state_dict(ref_vf.state_dict())
    assert tr.steps == (4, 5) and addresses == [b.data_ptr() for b in (tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf)]
    for opt, ref, count in ((opt_pf, ref_pf, 4.0), (opt_vf, ref_vf, 5.0)):
        got, want = opt.state_dict(), ref.state_dict()
        for i in want["state"]:
            assert float(got["state"][i]["step"]) == count
            assert torch.equal(got["state"][i]["exp_avg"], want["state"][i]["exp_avg"])
            assert torch.equal(got["state"][i]["exp_avg_sq"], want["state"][i]["exp_avg_sq"])
    # an empty state zeroes the moments and the count; other betas than the engine's are refused
    opt_pf.load_state_dict(torch.optim.Adam(pf.parameters(), lr=2e-4, eps=1e-5).state_dict())
    assert tr.steps == (0, 5) and not tr.m_pf.any() and not tr.v_pf.any() and tr.m_vf.any() and opt_pf.lr == 2e-4
    with pytest.raises(ValueError, match="betas"):
        opt_vf.load_state_dict(torch.optim.Adam(vf.parameters(), lr=2e-4, eps=1e-5, betas=(0.8, 0.999)).state_dict())
