"""CPU checks of the actor (no GPU): the fmaf twin against a float64 forward within rounding bounds, the packing of (W, b) lists and of
an nn.Sequential into gymnet_vecenv_actor_config's layout, the Python layer's argument checks, and the register budget of actor.hip's
kernels read from the gfx950 assembly (the runner's CartPole kernels must not spill), and the names of the actor_rollout_kernel forms in
that assembly against the recipe table of tests/_actor_forms.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _actor_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = (16, 50, 20, 2)


@pytest.mark.parametrize("widths", [RUNNER, (8, 13, 7, 3), (4, 2), (64, 64, 64, 64, 3)])
def test_twin_agrees_with_float64_within_rounding(widths):
    rng = np.random.default_rng(sum(widths))
    w, flat = twin.random_net(rng, list(widths))
    x = rng.normal(0, 1, (4096, widths[0])).astype(np.float32)
    logits, greedy = twin.forward(w, flat, x)
    ref, scale = twin.forward64(w, flat, x)
    # each fmaf rounds once: |error| <= (depth-weighted) u * sum |terms|, u = 2^-24, a few ulps per layer of the scale
    bound = 4 * len(widths) * max(widths) * 2.0 ** -24 * scale + 1e-30
    assert np.all(np.abs(logits.astype(np.float64) - ref) <= bound)
    assert np.array_equal(greedy, np.argmax(logits, axis=1))


def test_twin_is_a_single_rounding_chain():
    # 1 + 2^-24 * (1 + 2^-23) ... a product whose low bits decide the sum: fmaf keeps them, mul-then-add in float32 drops them
    w = np.array([1, 1], np.int32)
    a = np.float32(1.0 + 2.0 ** -12)
    flat = np.array([a, np.float32(-1.0)], np.float32)                  # W = a, b = -1
    logits, _ = twin.forward(w, flat, np.array([[a]], np.float32))
    exact = np.float64(a) * np.float64(a) - 1.0
    assert logits[0, 0] == np.float32(exact)
    assert np.float32(np.float32(a * a) - np.float32(1.0)) != logits[0, 0]


def _ve(gymnet):
    import importlib
    return importlib.import_module(gymnet.__name__ + ".vector_env")


def test_pack_weight_layout(gymnet):
    ve = _ve(gymnet)
    rng = np.random.default_rng(1)
    W0, b0 = rng.normal(size=(5, 3)).astype(np.float32), rng.normal(size=5).astype(np.float32)
    W1, b1 = rng.normal(size=(2, 5)).astype(np.float32), rng.normal(size=2).astype(np.float32)
    widths, flat = ve.actor_pack([(W0, b0), (W1, b1)])
    assert widths.tolist() == [3, 5, 2]
    assert np.array_equal(flat, np.concatenate([W0.ravel(), b0, W1.ravel(), b1]))
    torch = pytest.importorskip("torch")
    seq = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))
    widths2, flat2 = ve.actor_pack(seq)
    assert widths2.tolist() == [3, 5, 2]
    want = np.concatenate([seq[0].weight.detach().numpy().ravel(), seq[0].bias.detach().numpy(),
                           seq[2].weight.detach().numpy().ravel(), seq[2].bias.detach().numpy()])
    assert np.array_equal(flat2, want)
    # the twin of the packed Sequential is torch's forward up to rounding
    x = rng.normal(size=(64, 3)).astype(np.float32)
    logits, _ = twin.forward(widths2, flat2, x)
    assert np.allclose(logits, seq(torch.from_numpy(x)).detach().numpy(), rtol=1e-5, atol=1e-6)


def test_pack_rejects_bad_networks(gymnet):
    ve = _ve(gymnet)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        ve.actor_pack([])
    with pytest.raises(ValueError):
        ve.actor_pack([(np.zeros((5, 3), np.float32), np.zeros(4, np.float32))])          # b does not match W
    with pytest.raises(ValueError):
        ve.actor_pack([(np.zeros((5, 3), np.float32), np.zeros(5, np.float32)), (np.zeros((2, 4), np.float32), np.zeros(2, np.float32))])
    with pytest.raises(ValueError):
        ve.actor_pack(torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2)))  # no ReLU between
    with pytest.raises(ValueError):
        ve.actor_pack(torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU()))        # ends with a ReLU
    with pytest.raises(ValueError):
        ve.actor_pack(torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2)))


def test_capi_declares_the_actor_exports(gymnet):
    import importlib
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    for name in ("config", "load_device", "reset_device", "push_device", "act_device", "view"):
        assert "gymnet_vecenv_actor_" + name in capi.PROTOTYPES
    assert capi.ACTIONS_ACTOR == 3


@pytest.fixture(scope="module")
def actor_kernels():
    """{kernel name: resources} of actor.hip compiled to gfx950 assembly with the product's flags (tools/kernel_resources.py)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "actor.s")
        r = subprocess.run([kernel_resources.HIPCC] + kernel_resources.FLAGS + [os.path.join(kernel_resources.CSRC, "actor.hip"), "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return kernel_resources.kernels(out)


@pytest.mark.timeout(900)
def test_actor_kernels_do_not_spill(actor_kernels):
    k = actor_kernels
    names = [n for n in k if n.startswith("actor_")]
    assert any(n.startswith("actor_rollout_kernel<CartPole,") for n in names)
    for n in names:
        if n.startswith("actor_act_kernel") or n.startswith("actor_push_kernel") or n.startswith("actor_rollout_kernel<CartPole,"):
            assert k[n]["scratch"] == 0, (n, k[n])                     # the runner's shape: no spills
            assert k[n]["occupancy"] >= 2, (n, k[n])


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_rollout_kernel(actor_kernels):
    """tests/_actor_forms.py FORMS against the compiled set, by name: a 19th form, or one that is dropped, fails here"""
    import _actor_forms as forms
    compiled = sorted(n for n in actor_kernels if n.startswith("actor_rollout_kernel<"))
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 18
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
