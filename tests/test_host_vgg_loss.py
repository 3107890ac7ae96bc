"""CPU: the host side of models.losses.VGGPerceptualLoss -- its constructor (weights in both key layouts, the reference's
parameter names, frozen flags, key errors), the slice sampling, CombinedLoss with an assigned perceptual module, and the float64
restatement the GPU tests use as their truth (tests/vgg_restatement.py): which features are post-ReLU, and its gradient against
finite differences."""
import importlib

import pytest
import torch

from tests.vgg_restatement import CONV_INDICES, DEFAULT_LAYERS, Restatement, he_state_dict, slice_indices, smooth_volume, to_rgb


@pytest.fixture(scope="module")
def losses():
    return importlib.import_module("models.losses")


@pytest.fixture(scope="module")
def sd():
    return he_state_dict(7, upto=30)


# module index -> (block, index inside the block) for the default layer list, as the reference's ModuleList of slices names them
DEFAULT_NAMES = {0: (0, 0), 2: (0, 2), 5: (1, 2), 7: (1, 4), 10: (2, 2), 12: (2, 4), 14: (3, 1), 16: (3, 3), 19: (3, 6),
                 21: (3, 8), 23: (4, 1), 25: (4, 3), 28: (4, 6), 30: (4, 8)}


@pytest.mark.parametrize("prefix", ["", "features."])
def test_constructor_takes_both_key_layouts(losses, sd, prefix):
    weights = {prefix + k: v for k, v in sd.items()}
    weights["classifier.0.weight"] = torch.zeros(1)          # other keys of a whole-model state dict are ignored
    m = losses.VGGPerceptualLoss(weights=weights)
    assert isinstance(m, torch.nn.Module) and not m.training
    assert (m.feature_layers, m.use_l1, m.slice_sample_rate) == ([2, 7, 12, 21, 30], True, 0.2)
    params = dict(m.named_parameters())
    assert len(params) == 2 * len(DEFAULT_NAMES)
    for i, (b, j) in DEFAULT_NAMES.items():
        for kind in ("weight", "bias"):
            p = params[f"vgg_blocks.{b}.{j}.{kind}"]
            assert not p.requires_grad and p.dtype == torch.float32
            assert torch.equal(p, sd[f"{i}.{kind}"]), (i, kind)
    assert isinstance(m.vgg_blocks[0][0], torch.nn.Conv2d) and tuple(m.vgg_blocks[0][0].weight.shape) == (64, 3, 3, 3)
    assert tuple(m.vgg_blocks[4][8].weight.shape) == (512, 512, 3, 3)
    bufs = dict(m.named_buffers())
    assert set(bufs) == {"mean", "std"} and tuple(bufs["mean"].shape) == (1, 3, 1, 1)
    assert torch.equal(bufs["mean"].flatten(), torch.tensor([0.485, 0.456, 0.406]))
    assert torch.equal(bufs["std"].flatten(), torch.tensor([0.229, 0.224, 0.225]))
    assert set(m.state_dict()) == set(params) | {"mean", "std"}


def test_weights_from_a_file(losses, sd, tmp_path):
    path = tmp_path / "vgg19_features.pt"
    torch.save(sd, path)
    for arg in (path, str(path)):
        m = losses.VGGPerceptualLoss(weights=arg, use_l1=False, slice_sample_rate=0.5)
        assert torch.equal(m.vgg_blocks[1][4].weight, sd["7.weight"]) and m.use_l1 is False


def test_only_the_needed_convs_are_required(losses, sd):
    short = {k: v for k, v in sd.items() if int(k.split(".")[0]) <= 16}
    m = losses.VGGPerceptualLoss(feature_layers=[3, 8, 17], weights=short)
    names = [n for n, _ in m.named_parameters() if n.endswith("weight")]
    assert names == ["vgg_blocks.0.0.weight", "vgg_blocks.0.2.weight", "vgg_blocks.1.1.weight", "vgg_blocks.1.3.weight",
                     "vgg_blocks.2.1.weight", "vgg_blocks.2.3.weight", "vgg_blocks.2.5.weight", "vgg_blocks.2.7.weight"]
    assert isinstance(m.vgg_blocks[0][3], torch.nn.ReLU) and m.vgg_blocks[0][3].inplace and len(m.vgg_blocks[2]) == 9
    with pytest.raises(ValueError, match="'features.19.weight'"):
        losses.VGGPerceptualLoss(weights=short)


def test_key_errors_name_the_key(losses, sd):
    for key in ("0.weight", "12.bias", "30.weight"):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=f"'features.{key}'.*missing"):
            losses.VGGPerceptualLoss(weights=bad)
    bad = dict(sd)
    bad["7.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(ValueError, match=r"'7.weight' has shape \(128, 64, 3, 3\), expected \(128, 128, 3, 3\)"):
        losses.VGGPerceptualLoss(weights=bad)
    bad = {"features." + k: v for k, v in sd.items()}
    bad["features.21.bias"] = torch.zeros(256)
    with pytest.raises(ValueError, match=r"'features.21.bias' has shape \(256,\)"):
        losses.VGGPerceptualLoss(weights=bad)
    with pytest.raises(ValueError, match="state dict or a path"):
        losses.VGGPerceptualLoss(weights=3)
    for layers in ([], [7, 2], [2, 2], [2, 37], [-1, 2], [2.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            losses.VGGPerceptualLoss(feature_layers=layers, weights=sd)


def test_without_weights_it_still_raises(losses):
    with pytest.raises(NotImplementedError, match="torchvision"):
        losses.VGGPerceptualLoss()
    with pytest.raises(NotImplementedError, match="lambda_perceptual=0"):
        losses.VGGPerceptualLoss(feature_layers=[2], use_l1=False, slice_sample_rate=1.0, weights=None)


@pytest.mark.parametrize("depth", [1, 4, 5, 48])
@pytest.mark.parametrize("rate", [0.2, 0.5, 1.0])
def test_slice_indices_are_the_linspace_call(losses, sd, depth, rate):
    m = losses.VGGPerceptualLoss(feature_layers=[2], weights=sd, slice_sample_rate=rate)
    num = max(1, int(depth * rate))
    want = torch.linspace(0, depth - 1, num, dtype=torch.long) if num < depth else torch.arange(depth)
    got = m.slice_indices(depth)
    assert got.dtype == torch.long and torch.equal(got, want) and torch.equal(slice_indices(depth, rate), want)
    assert len(set(got.tolist())) == got.numel()           # distinct: the backward scatters without accumulation
    # the restatement's gather is the same indexing
    x = torch.arange(depth, dtype=torch.float64).view(1, 1, depth, 1, 1).expand(2, 1, depth, 16, 16)
    rgb = to_rgb(x, rate)
    back = rgb[:, 0, 0, 0] * 0.229 + 0.485                  # (x + 1) / 2
    assert torch.allclose(back * 2 - 1, want.double().repeat(2), atol=1e-12)


def test_edge_cases_without_a_device(losses, sd, pkg):
    m = losses.VGGPerceptualLoss(feature_layers=[2], weights=sd)
    with pytest.raises(AssertionError, match=r"Expected grayscale input \(C=1\)"):
        m(torch.zeros(1, 2, 4, 32, 32), torch.zeros(1, 2, 4, 32, 32))
    with pytest.raises(ValueError, match="multiples of 16"):
        m(torch.zeros(1, 1, 4, 24, 32), torch.zeros(1, 1, 4, 24, 32))
    with pytest.raises(ValueError, match="multiples of 16"):
        m(torch.zeros(1, 1, 4, 32, 40), torch.zeros(1, 1, 4, 32, 40))
    with pytest.raises(ValueError, match="shape mismatch"):
        m(torch.zeros(1, 1, 4, 32, 32), torch.zeros(1, 1, 4, 32, 48))
    with pytest.raises(ValueError, match=r"\(B, 1, D, H, W\)"):
        m(torch.zeros(1, 32, 32), torch.zeros(1, 32, 32))
    with pytest.raises(pkg.CtsiError, match="no CPU path"):
        m(torch.zeros(1, 1, 4, 32, 32), torch.zeros(1, 1, 4, 32, 32))


class _StandIn(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value, self.calls = value, 0

    def forward(self, pred, target):
        self.calls += 1
        return pred.new_tensor(self.value) + 0.0 * pred.sum()


def test_combined_loss_calls_an_assigned_perceptual_module_on_schedule(losses):
    c = losses.CombinedLoss(lambda_perceptual=0.5, lambda_ssim=0.25, perceptual_every_n_steps=2, ssim_every_n_steps=3)
    c.perceptual_loss, c.ssim_loss = _StandIn(0.5), _StandIn(0.25)
    pred = torch.zeros(1, 1, 2, 32, 32, requires_grad=True)
    target = torch.zeros(1, 1, 2, 32, 32)
    for step in range(7):
        total, d = c(pred, target, torch.tensor(1.0, requires_grad=True))
        want = {"diffusion", "total"} | ({"perceptual"} if step % 2 == 0 else set()) | ({"ssim"} if step % 3 == 0 else set())
        assert set(d) == want and int(c.step) == step + 1
        assert d["total"] == pytest.approx(1.0 + (0.25 if step % 2 == 0 else 0.0) + (0.0625 if step % 3 == 0 else 0.0))
        assert total.requires_grad
    assert c.perceptual_loss.calls == 4 and c.ssim_loss.calls == 3
    assert "perceptual_loss.value" not in c.state_dict()
    # a real module is a submodule: its frozen weights travel with the CombinedLoss
    c.perceptual_loss = losses.VGGPerceptualLoss(feature_layers=[2], weights=he_state_dict(3, upto=2))
    assert "perceptual_loss.vgg_blocks.0.2.weight" in c.state_dict()
    assert not any(p.requires_grad for p in c.parameters())


def test_restatement_features_are_post_relu_but_the_last(sd):
    r = Restatement(sd, DEFAULT_LAYERS)
    x = smooth_volume((1, 1, 2, 32, 32), 11).double()
    feats = r.features(to_rgb(x, 1.0))
    assert [f.shape[1] for f in feats] == [64, 128, 256, 512, 512] and [f.shape[-1] for f in feats] == [32, 16, 8, 4, 2]
    for f in feats[:4]:
        assert float(f.min()) >= 0.0 and float(f.max()) > 0.0
    assert float(feats[4].min()) < 0.0
    # ReLU-ended blocks are post-ReLU throughout, and the stack ends early
    r2 = Restatement(sd, (3, 8, 17))
    feats = r2.features(to_rgb(x, 1.0))
    assert all(float(f.min()) >= 0.0 for f in feats) and [f.shape[1] for f in feats] == [64, 128, 256]
    assert CONV_INDICES[:14] == tuple(sorted(DEFAULT_NAMES))


@pytest.mark.parametrize("use_l1", [True, False])
def test_restatement_gradient_matches_finite_differences(sd, use_l1):
    r = Restatement(sd, DEFAULT_LAYERS, use_l1=use_l1, rate=1.0)
    # no clamped plateaus here: on a flat region neighbouring conv outputs are EQUAL, max pooling then sits exactly on a kink
    # (autograd takes the first maximum's derivative, a central difference the mean of the tied ones)
    g = torch.Generator().manual_seed(21)
    pred = (0.4 * torch.randn(1, 1, 2, 16, 16, generator=g, dtype=torch.float64)).requires_grad_(True)
    target = 0.4 * torch.randn(1, 1, 2, 16, 16, generator=g, dtype=torch.float64)
    loss = r(pred, target)
    (grad,) = torch.autograd.grad(loss, pred)
    assert float(grad.abs().max()) > 0.0
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for _ in range(6):                      # directional derivatives: central differences along random directions
        v = torch.randn(pred.shape, generator=g, dtype=torch.float64)
        eps = 1e-6
        with torch.no_grad():
            fd = (r(pred + eps * v, target) - r(pred - eps * v, target)) / (2 * eps)
        an = (grad * v).sum()
        worst = max(worst, abs(float(fd - an)) / max(abs(float(an)), 1e-12))
    # the loss is piecewise smooth (ReLU, max pooling, |.|): a kink inside +-eps along a direction is rare but possible, so the
    # bar is that of a first-order scheme on such a function, far below any wrong-formula error (O(1))
    assert worst < 1e-4, worst
