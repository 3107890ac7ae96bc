"""CPU: the torch restatement of the MS-SSIM loss (tests/msssim_restatement.py) reproduces the reference's own class on the
stored golden cases (tests/golden/msssim_v1.npz, written by make_golden_msssim.py): loss to 1e-6 absolute, level means, the
full `pred` gradient to 1e-5 rel-L2, NaN where the reference gives NaN.  This pins the yardstick of the GPU tests."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel_l2
from tests.msssim_restatement import msssim_loss, window_2d

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msssim_v1.npz")
CASES = ("b2", "c2", "nan", "noisy", "odd")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def test_fixture_is_complete_and_away_from_the_pole(gold):
    assert tuple(gold["cases"]) == CASES
    for tag in CASES:
        means = gold[f"{tag}.means"]
        if tag == "nan":
            assert np.isnan(gold[f"{tag}.loss"]) and (means < 0).any() and np.isnan(gold[f"{tag}.grad"]).all()
        else:
            assert (means >= 0.05).all(), (tag, means)


def test_window_bit_equal(gold):
    assert torch.equal(window_2d(11)[None, None], torch.from_numpy(gold["window"]))


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(gold, tag):
    pred = torch.from_numpy(gold[f"{tag}.pred"]).requires_grad_(True)
    target = torch.from_numpy(gold[f"{tag}.target"])
    loss, means = msssim_loss(pred, target, torch.float32, return_means=True)
    loss.backward()
    if tag == "nan":
        assert torch.isnan(loss) and torch.isnan(pred.grad).all()
        return
    e_loss = abs(loss.item() - float(gold[f"{tag}.loss"]))
    e_means = np.abs(means.detach().numpy().astype(np.float64) - gold[f"{tag}.means"]).max()
    e_grad = rel_l2(pred.grad, torch.from_numpy(gold[f"{tag}.grad"]))
    print(f"[{tag}] loss err {e_loss:.3g}  means err {e_means:.3g}  grad rel-L2 {e_grad:.3g}")
    assert e_loss <= 1e-6 and e_means <= 1e-6 and e_grad <= 1e-5
