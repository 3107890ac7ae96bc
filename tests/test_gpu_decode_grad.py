"""GPU: `SliceInterpolationVAE.decode_with_grad` (vae_train_engine.VAEDecodeGradProgram): a decode of a frozen
VAE that is differentiable in the latent.

Yardstick (as tests/test_gpu_vae_train.py): grad_z against the fp32 oracle's decoder under torch autograd, the error held
against the oracle's own under bf16 autocast:  err_hip <= 2 * err_autocast + 2e-2  (rel-L2).  The forward is `_decode(z, "bf16")`
bit for bit; no parameter gets a gradient; the program holds no weight-gradient launch; a stale backward raises."""
import pytest
import torch

from oracle import ref_ops as R
from tests.helpers import formula_input, load_formula, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SF = 0.5
SHAPES = [(2, 8, 3, 5, 6), (1, 8, 2, 3, 3)]


@pytest.fixture(scope="module")
def tiny(pkg):
    vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=16, scaling_factor=SF)
    sd = load_formula(vae, 50)
    vae.to(DEV)
    yield vae, sd
    vae.invalidate_engine_cache()


def _inputs(shape):
    z = formula_input(shape, 61)
    n, _, d, h, w = shape
    target = formula_input((n, 1, d, 4 * h, 4 * w), 62).clamp(-1, 1)
    return z, target


def _oracle_grad(sd, z, target, autocast):
    zz = z.clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            recon = R.vae_decode(sd, zz, SF)
    else:
        recon = R.vae_decode(sd, zz, SF)
    (recon.float() - target).pow(2).mean().backward()
    return zz.grad.detach().float()


def _programs(vae):
    return [p for k, p in vae.decoder.__dict__.get("_ctsi_programs", {}).items() if k[0] == "dec-grad"]


@pytest.mark.parametrize("shape", SHAPES, ids=["2x3x5x6", "1x2x3x3"])
def test_forward_bits_and_grad_z(tiny, shape):
    vae, sd = tiny
    z, target = _inputs(shape)
    zd = z.to(DEV).requires_grad_(True)
    flags = [p.requires_grad for p in vae.parameters()]
    recon = vae.decode_with_grad(zd)
    assert recon.grad_fn is not None and tuple(recon.shape) == tuple(target.shape)
    with torch.no_grad():
        assert torch.equal(recon.detach(), vae._decode(zd.detach(), "bf16"))
    (recon - target.to(DEV)).pow(2).mean().backward()
    torch.cuda.synchronize()
    ref, ac = _oracle_grad(sd, z, target, False), _oracle_grad(sd, z, target, True)
    e_hip, e_ac = rel_l2(zd.grad.cpu(), ref), rel_l2(ac, ref)
    print(f"  grad_z {shape}: hip {e_hip:.3e} autocast {e_ac:.3e} ratio {e_hip / (2 * e_ac + 2e-2):.2f}")
    assert e_hip <= 2 * e_ac + 2e-2
    # frozen: no parameter gradient, the flags as they were, no weight-gradient launch in the program
    assert all(p.grad is None for p in vae.parameters())
    assert [p.requires_grad for p in vae.parameters()] == flags
    progs = _programs(vae)
    assert progs
    for prog in progs:
        names = [m[0] for m in prog.op_meta]
        assert not [nm for nm in names if "wgrad" in nm or "bgrad" in nm], names
        assert "seam.grad_z" in names and "head.grad" in names


def test_requires_grad_flags_are_not_read(tiny):
    """The same result with every parameter's requires_grad switched off (the way a training script freezes the VAE)."""
    vae, _ = tiny
    z, target = _inputs(SHAPES[1])
    grads = []
    for flag in (True, False):
        for p in vae.parameters():
            p.requires_grad_(flag)
        zd = z.to(DEV).requires_grad_(True)
        (vae.decode_with_grad(zd) - target.to(DEV)).pow(2).mean().backward()
        grads.append(zd.grad.clone())
        assert [p.requires_grad for p in vae.parameters()] == [flag] * len(list(vae.parameters()))
    for p in vae.parameters():
        p.requires_grad_(True)
    assert torch.equal(grads[0], grads[1])          # (also: two identical runs give identical bits)


def test_programs_are_cached_per_shape_and_fall_through(tiny, pkg):
    vae, _ = tiny
    vae.invalidate_engine_cache()
    for shape in SHAPES + SHAPES:
        z, target = _inputs(shape)
        zd = z.to(DEV).requires_grad_(True)
        vae.decode_with_grad(zd).sum().backward()
    assert len(_programs(vae)) == 2
    # no gradient wanted: the plain bf16 decode, no new program, no autograd node
    z, _ = _inputs(SHAPES[0])
    out = vae.decode_with_grad(z.to(DEV))
    assert out.grad_fn is None and len(_programs(vae)) == 2
    with torch.no_grad():
        out2 = vae.decode_with_grad(z.to(DEV).requires_grad_(True))
    assert out2.grad_fn is None and torch.equal(out, out2)
    with pytest.raises(pkg.CtsiError, match="ROCm"):
        vae.decode_with_grad(z.requires_grad_(True))


def test_generation_guard(tiny, pkg):
    vae, _ = tiny
    z, target = _inputs(SHAPES[1])
    z1, z2 = z.to(DEV).requires_grad_(True), (0.5 * z).to(DEV).requires_grad_(True)
    r1 = vae.decode_with_grad(z1)
    r2 = vae.decode_with_grad(z2)
    with pytest.raises(pkg.CtsiError, match="overwritten"):
        r1.sum().backward()
    r2.sum().backward()              # the newest forward's backward is fine
    assert z2.grad is not None and z1.grad is None
