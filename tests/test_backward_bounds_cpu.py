"""CPU self-checks of what the wide-row backward tests on the GPU rely on: the reworked min / max case builders still make
the width-64 tensors they always made, and the fp64-oracle bound of the sum == "add" backward test (tests/add_backward.py)
is one that a correct fp32 implementation -- the C oracle's own fp32 backward -- meets on every chosen case."""
import pytest
import torch

from tests import add_backward, helpers
from tests import test_minmax_backward_gpu as minmax

MULS = ["mul", "add"]

# helpers.fingerprint (first 16 hex digits) of edges, x, rel (and x_add) of CASES[name](manual_seed(index in sorted order)),
# recorded from the builders before they took a `width`
WIDTH_64_FINGERPRINTS = {"all_negative": "f554a28881a37339", "copies": "aadad553dea24630", "empty": "5a962d0b090c2c10",
                         "hub": "68ce2e766ab600fd", "relu_zeros": "57cd36fc01283bf8", "signed_zeros": "f325a8c6196dd583"}


def _tensors(spec):
    return list(spec["edges"]) + [spec["x"], spec["rel"]] + ([spec["x_add"]] if "x_add" in spec else [])


@pytest.mark.parametrize("name", sorted(minmax.CASES))
def test_case_builders_at_width_64_are_bit_identical(name):
    seed = sorted(minmax.CASES).index(name)
    spec = minmax.CASES[name](torch.Generator().manual_seed(seed))
    assert helpers.fingerprint(*_tensors(spec))[:16] == WIDTH_64_FINGERPRINTS[name]
    same = minmax.CASES[name](torch.Generator().manual_seed(seed), width=64)
    assert helpers.fingerprint(*_tensors(same))[:16] == WIDTH_64_FINGERPRINTS[name]
    # a wider case: the same edges and first 64 columns, the case's structure in the new columns too
    wide = minmax.CASES[name](torch.Generator().manual_seed(seed), width=200)
    assert all(torch.equal(a, b) for a, b in zip(wide["edges"], spec["edges"]))
    for k in ("x", "rel"):
        assert wide[k].shape[1] == 200 and torch.equal(wide[k][:, :64], spec[k])
        assert torch.equal((wide[k][:, 64:] == 0).all(1), (spec[k] == 0).all(1)), "zero rows are zero at every width"


def test_tiny_case_fits_a_batch_of_a_thousand():
    spec = minmax.case_tiny(torch.Generator().manual_seed(17), width=72)
    assert spec["x"].shape == (12, 72) and spec["edges"][0].numel() == 60
    assert 1100 * 60 * 72 * 8 < 64 << 20        # one (batch, E, d) fp64 temporary of the restatement


@pytest.mark.parametrize("case", add_backward.CASES)
@pytest.mark.parametrize("mul", MULS)
@pytest.mark.parametrize("dtype,dim", add_backward.SHAPES)
def test_oracle_in_working_precision_meets_the_add_backward_bound(case, mul, dtype, dim):
    """The reference alone passes the bound the GPU is held to: the oracle's backward in the working precision against its
    fp64 backward, every layout and weighting of test_add_backward_matches_fp64_oracle (and the seed of the unaligned one)."""
    for seed in (0, 1):
        for layout in add_backward.LAYOUTS:
            for weights in add_backward.WEIGHTS:
                ops = add_backward.make_operands(case, dim, dtype, layout, weights, mul, seed=seed)
                wg, rg, xg = add_backward.oracle_backward(ops, dtype)
                total = xg + ops["base"]
                if weights == "keep":       # the engine's convention for a keep mask: a dropped edge has no weight gradient
                    wg = wg * (ops["w"] != 0)
                try:
                    add_backward.check(ops, dtype, wg, rg.sum(0) if layout == "shared" else rg, xg, got_total=total)
                except AssertionError as e:
                    raise AssertionError("%s / %s: %s" % (layout, weights, e))


def test_score_scale_of_the_training_steps_at_other_hidden_sizes():
    """test_train_mode_step_at_other_hidden_sizes_matches_cpu_oracle holds scores and loss to TOL and 1e-5 times
    max(1, max |score|).  That factor is 1 for the hidden-32 and hidden-128 models; for hidden 48 / TransE / no LayerNorm it
    is about 54, the CPU oracle's own fp32 path misses the absolute figures against its fp64 path, and meets the scaled ones."""
    from tests import test_models_gpu as mg
    data, filtered, neg = mg.train_step_inputs()
    for config in mg.OTHER_HIDDEN_SIZES:
        state, cfg = mg.random_model(*config)
        loss32, pred32, _ = mg.cpu_train_step(state, cfg, data, filtered, neg, torch.float32)
        loss64, pred64, _ = mg.cpu_train_step(state, cfg, data, filtered, neg, torch.float64)
        scale = max(1.0, pred32.abs().max().item())
        err, loss_err = (pred32.double() - pred64).abs().max().item(), abs(loss32 - loss64)
        print("hidden %d: max |score| %.4g, cpu fp32 - fp64: scores %.3g, loss %.3g" % (config[0], pred32.abs().max().item(), err, loss_err))
        if config[0] == 48:
            assert 50 < scale < 60 and err > mg.TOL and loss_err > 1e-5
        else:
            assert scale == 1.0
        assert err <= mg.TOL * scale and loss_err <= 1e-5 * scale
