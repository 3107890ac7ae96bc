"""CPU: ema.EMAWeights on CPU parameters (the plain torch path: lerp_, tensor swap) -- the decay schedule, the recurrence,
applied(), the state dict and use_ema checkpoint loading.  Everything here except the kernels is what the device path runs too."""
import importlib

import pytest
import torch

pkg = importlib.import_module("video-to-video-diffusion_amd")
ckpt_mod = importlib.import_module("video-to-video-diffusion_amd.checkpoint")
EMAWeights, CtsiError = pkg.EMAWeights, pkg.CtsiError


def _net(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    net[2].bias.requires_grad_(False)                          # a frozen parameter gets no shadow
    return net


def test_decay_schedule_and_crossover():
    for decay in (0.9999, 0.999, 0.95):
        ema = EMAWeights(_net(), decay=decay)
        for n in (0, 1, 2, 9, 10, 100, 1000, 89989, 89990, 89991, 10 ** 6):
            assert ema.decay_at(n) == min(decay, (1.0 + n) / (10.0 + n))
        assert ema.decay_at(0) == 0.1
        # (1 + n) / (10 + n) >= decay  <=>  n >= (10 decay - 1) / (1 - decay): 89 990 for 0.9999
        cross = (10.0 * decay - 1.0) / (1.0 - decay)
        first = next(n for n in range(int(cross) - 2, int(cross) + 3) if (1.0 + n) / (10.0 + n) >= decay)
        assert abs(first - cross) < 1.0 + 1e-6 * cross and first >= cross - 1e-6 * cross
        assert ema.decay_at(first - 1) < decay and ema.decay_at(first) == decay and ema.decay_at(first + 1000) == decay
    assert round((10.0 * 0.9999 - 1.0) / (1.0 - 0.9999)) == 89990
    flat = EMAWeights(_net(), decay=0.99, warmup=False)
    assert flat.decay_at(0) == flat.decay_at(5) == 0.99
    with pytest.raises(ValueError):
        EMAWeights(_net(), decay=1.0)


def test_k_updates_follow_the_float64_recurrence():
    k = 40
    net = _net(1)
    ema = EMAWeights(net, decay=0.999)
    params = [p for p in net.parameters() if p.requires_grad]
    ref = [p.detach().double().clone() for p in params]
    gen = torch.Generator().manual_seed(7)
    largest = [float(r.abs().max()) for r in ref]
    for n in range(k):
        with torch.no_grad():
            for i, p in enumerate(params):                     # a fixed sequence of parameter values
                p.copy_(torch.randn(p.shape, generator=gen) * (1.0 + 0.1 * n))
                largest[i] = max(largest[i], float(p.abs().max()))
        ema.update()
        w = 1.0 - ema.decay_at(n)
        for r, p in zip(ref, params):
            r += w * (p.detach().double() - r)
    assert ema.num_updates == k
    # each fp32 lerp rounds once or twice: k updates stay within k * 2^-23 of the float64 recurrence, relative to the largest
    # magnitude that went through it
    bound = k * 2.0 ** -23
    for name, r, big in zip(ema.names, ref, largest):
        s = ema.state_dict()['shadow'][name]
        assert s.dtype == torch.float32
        err = float((s.double() - r).abs().max())
        print(f"{name}: max error {err:.3e}, bound {bound * big:.3e}")
        assert err <= bound * big, name


def test_applied_swaps_and_restores_bit_exactly():
    net = _net(2)
    ema = EMAWeights(net, decay=0.9)
    params = [p for p in net.parameters() if p.requires_grad]
    with torch.no_grad():
        for p in params:
            p.add_(torch.randn_like(p))
    ema.update()
    raw = [p.detach().clone() for p in params]
    avg = [s.clone() for s in ema.state_dict()['shadow'].values()]
    assert not any(torch.equal(a, b) for a, b in zip(raw, avg))
    ptrs = [p.data_ptr() for p in params]
    frozen = net[2].bias.detach().clone()
    v0 = params[0]._version
    with ema.applied() as inside:
        assert inside is ema
        assert all(torch.equal(p.detach(), a) for p, a in zip(params, avg))     # the model holds the averaged weights
        assert params[0]._version > v0
        with pytest.raises(CtsiError, match="nested"):
            with ema.applied():
                pass
        with pytest.raises(CtsiError, match="applied"):
            ema.update()
        with pytest.raises(CtsiError, match="applied"):
            ema.state_dict()
        assert all(torch.equal(p.detach(), a) for p, a in zip(params, avg))     # the refused calls changed nothing
    assert all(torch.equal(p.detach(), r) for p, r in zip(params, raw))         # restored bit for bit
    assert all(torch.equal(s, a) for s, a in zip(ema.state_dict()['shadow'].values(), avg))
    assert [p.data_ptr() for p in params] == ptrs and torch.equal(net[2].bias.detach(), frozen)
    assert ema.num_updates == 1
    with pytest.raises(RuntimeError, match="boom"):                             # an exception inside still restores
        with ema.applied():
            raise RuntimeError("boom")
    assert all(torch.equal(p.detach(), r) for p, r in zip(params, raw))
    ema.update()                                                                # and the instance is usable again
    assert ema.num_updates == 2


class _FakeFused:
    pass


def test_attached_instance_refuses_an_explicit_update():
    ema = EMAWeights(_net(3))
    opt = _FakeFused()
    ema._attach(opt)
    with pytest.raises(CtsiError, match="attached to a fused optimizer"):
        ema.update()
    with pytest.raises(CtsiError, match="another optimizer"):
        ema._attach(_FakeFused())
    # the optimizer's side of the contract, on the CPU path: the launch covered the first parameter, the rest follow here
    params = ema.params
    before = [s.clone() for s in ema.shadows]
    with torch.no_grad():
        for p in params:
            p.mul_(2.0)
    w = ema._fused_weight()
    assert w == 1.0 - ema.decay_at(0)
    ema._fused_done(params[:1], w)
    assert ema.num_updates == 1 and torch.equal(ema.shadows[0], before[0])      # (the kernel would have moved it)
    for s, b, p in zip(ema.shadows[1:], before[1:], params[1:]):
        assert torch.equal(s, b.clone().lerp_(p.detach(), w))
    with ema.applied():
        with pytest.raises(CtsiError, match="applied"):
            ema._fused_weight()                                                 # what FusedAdamW.step() asks first


def test_state_dict_round_trip_and_names():
    net = _net(4)
    ema = EMAWeights(net, decay=0.99, prefix='net.')
    trainable = ['net.' + n for n, p in net.named_parameters() if p.requires_grad]
    assert ema.names == trainable and 'net.2.bias' not in ema.names
    assert set(EMAWeights(net).names) <= set(net.state_dict())                  # no prefix: keys of the module's state dict
    it = iter(net.named_parameters())
    assert EMAWeights(it, prefix='x.').names == ['x.' + n[len('net.'):] for n in trainable]
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
    ema.update()
    ema.update()
    sd = ema.state_dict()
    assert set(sd) == {'decay', 'warmup', 'num_updates', 'shadow'} and sd['num_updates'] == 2 and sd['decay'] == 0.99
    assert list(sd['shadow']) == trainable
    other = EMAWeights(_net(5), decay=0.5, warmup=False, prefix='net.')
    ptrs = [s.data_ptr() for s in other.shadows]
    other.load_state_dict({**sd, 'shadow': {k: v.clone() for k, v in sd['shadow'].items()}})
    assert (other.decay, other.warmup, other.num_updates) == (0.99, True, 2)
    assert [s.data_ptr() for s in other.shadows] == ptrs                        # loaded in place
    assert all(torch.equal(a, b) for a, b in zip(other.shadows, ema.shadows))
    bad = dict(sd, shadow={k: v for k, v in list(sd['shadow'].items())[1:]})
    with pytest.raises(CtsiError, match="names"):
        other.load_state_dict(bad)
    bad = dict(sd, shadow={**sd['shadow'], 'net.0.bias': torch.zeros(6)})
    with pytest.raises(CtsiError, match="shape"):
        other.load_state_dict(bad)
    # model.load_state_dict(sd['shadow'], strict=False) works when the names are keys of the model's state dict
    plain = EMAWeights(net)
    twin = _net(6)
    missing, unexpected = twin.load_state_dict(plain.state_dict()['shadow'], strict=False)
    assert unexpected == [] and missing == ['2.bias']


def test_use_ema_checkpoint_loading(tmp_path):
    from tests.helpers import TINY_CFG
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    for p in model.vae.parameters():
        p.requires_grad_(False)
    ema = EMAWeights(model.unet, decay=0.9, prefix='unet.')
    assert set(ema.names) <= set(model.state_dict()) and set(EMAWeights(model).names) == set(ema.names)
    with torch.no_grad():
        for p in model.unet.parameters():
            p.add_(0.01 * torch.randn_like(p))
    ema.update()
    path = str(tmp_path / "checkpoint_best_epoch_1.pt")
    model.save_checkpoint(path, epoch=1, ema_state_dict=ema.state_dict())
    raw = {k: v.clone() for k, v in model.state_dict().items()}
    shadow = {k: v.clone() for k, v in ema.state_dict()['shadow'].items()}

    m_raw, meta = ckpt_mod.load_model_from_checkpoint(pkg.VideoToVideoDiffusion(TINY_CFG), path, device='cpu')
    assert meta['epoch'] == 1 and all(torch.equal(v, raw[k]) for k, v in m_raw.state_dict().items())
    m_ema, _ = ckpt_mod.load_model_from_checkpoint(pkg.VideoToVideoDiffusion(TINY_CFG), path, device='cpu', use_ema=True)
    differs = 0
    for k, v in m_ema.state_dict().items():
        assert torch.equal(v, shadow[k] if k in shadow else raw[k]), k
        differs += int(k in shadow and not torch.equal(v, raw[k]))
    assert differs > 10

    resumed = EMAWeights(m_raw.unet, prefix='unet.')                             # a trainer resuming its average
    resumed.load_state_dict(torch.load(path, weights_only=False)['ema_state_dict'])
    assert resumed.num_updates == 1 and all(torch.equal(s, shadow[n]) for n, s in zip(resumed.names, resumed.shadows))

    plain = str(tmp_path / "checkpoint_best_epoch_2.pt")
    model.save_checkpoint(plain, epoch=2)
    with pytest.raises(KeyError, match="ema_state_dict"):
        ckpt_mod.load_model_from_checkpoint(pkg.VideoToVideoDiffusion(TINY_CFG), plain, device='cpu', use_ema=True)
    stray = ema.state_dict()
    stray['shadow'] = {**stray['shadow'], 'unet.no_such.weight': torch.zeros(1)}
    model.save_checkpoint(plain, epoch=2, ema_state_dict=stray)
    with pytest.raises(KeyError, match="no_such"):
        ckpt_mod.load_model_from_checkpoint(pkg.VideoToVideoDiffusion(TINY_CFG), plain, device='cpu', use_ema=True)
