"""The training plans run the conv stack's BatchNorm1-backward sums and the spatial-conv weight gradient as ONE recompute (eegclip_cstack_bwd_stats_w2, its slabs
reduced by eegclip_cstack_w2_reduce beside the taps reduction): the op list of the backward plan, and one step through the single-submission step plan against
the launch-by-launch step from the same snapshot (the construction and the tolerances of tests/test_product_on_emulator.py's step-plan test), on the emulator."""
import copy

import numpy as np
import pytest
import torch

from conftest import SEED
from emu_patch import product_on_emulator
from eeg_image_decode_amd import synthetic as syn
from oracle import atms as oatms

pytestmark = pytest.mark.emu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def make_model(state_np):
    from eeg_image_decode_amd.atms import ATMS
    m = ATMS()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state_np.items()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def test_backward_plan_takes_sums_and_weight_gradient_from_one_recompute(monkeypatch):
    B, NC = 16, 40           # (a batch the plan takes: four sample groups of the row-major kernel)
    cls = T(syn.unit_features(SEED + 4, NC, tag="c"))
    rng = np.random.default_rng(1)
    data = [(T(syn.eeg_batch(SEED + 100 + i, B)), T(syn.unit_features(SEED + 200 + i, B, tag="i")), T(syn.unit_features(SEED + 300 + i, B, tag="t")),
             T(rng.integers(0, NC, size=B).astype(np.int64))) for i in range(3)]

    def new_model():
        return make_model(syn.make_state(SEED, oatms.state_spec())).train()

    with product_on_emulator():
        from eeg_image_decode_amd import optim, retrieval, step_plan
        monkeypatch.setattr(step_plan, "_runtime_ok", lambda: True)
        monkeypatch.setattr(step_plan, "_on_device", lambda t: True)
        monkeypatch.setattr(step_plan.StepPlan, "WARM_STEPS", 2)
        torch.manual_seed(5)
        m = new_model()
        opt = optim.AdamW(m.parameters(), lr=3e-4)
        acc, correct = [], torch.zeros(1, dtype=torch.int32)
        for x, img, txt, lab in data[:2]:
            retrieval.contrastive_step(m, opt, x, 1, img, txt, lab, cls, acc, correct, alpha=0.99, objective="retrieval")
        assert not retrieval.step_plans_of(m)
        snap = (copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict()), torch.get_rng_state(), correct.clone())
        x, img, txt, lab = data[2]
        f_plan = retrieval.contrastive_step(m, opt, x, 1, img, txt, lab, cls, acc, correct, alpha=0.99, objective="retrieval")
        plans = retrieval.step_plans_of(m)
        assert len(plans) == 1 and isinstance(plans[0], step_plan.StepPlan)
        for names in (plans[0].bwd.op_names(), plans[0].pl.op_names()):
            assert names.count("eegclip_cstack_bwd_stats_w2") == 1, names
            assert "eegclip_cstack_bwd_stats" not in names and "eegclip_cstack_bwd_w2" not in names
            assert names.count("eegclip_cstack_bwd_apply") == 1 and names.count("eegclip_cstack_w2_reduce") == 1
            # sums before the apply pass; the slab reduction right behind the taps reduction (one fork), both behind the apply pass
            i_sw, i_ap, i_tp, i_w2 = (names.index("eegclip_cstack_" + k) for k in ("bwd_stats_w2", "bwd_apply", "bwd_taps_reduce", "w2_reduce"))
            assert i_sw < i_ap < i_tp and i_w2 == i_tp + 1
        # (in the step plan the two reductions stand in front of the early optimizer update)
        names = plans[0].pl.op_names()
        assert "eegclip_adamw_step_zero_grad" in names[names.index("eegclip_cstack_w2_reduce"):]
        res_plan = ({k: p.detach().clone() for k, p in m.named_parameters()}, float(acc[-1]), int(correct), f_plan.clone(),
                    {k: v.clone() for k, v in m.state_dict().items() if "running" in k})
        monkeypatch.setenv("EEGCLIP_STEP_PLAN", "0")
        m2 = new_model()
        m2.load_state_dict(snap[0])
        opt2 = optim.AdamW(m2.parameters(), lr=3e-4)
        opt2.load_state_dict(snap[1])
        torch.set_rng_state(snap[2])
        acc2, correct2 = [], snap[3].clone()
        f_ord = retrieval.contrastive_step(m2, opt2, x, 1, img, txt, lab, cls, acc2, correct2, alpha=0.99, objective="retrieval")
        assert not retrieval.step_plans_of(m2)
    np.testing.assert_allclose(res_plan[3].numpy(), f_ord.numpy(), atol=2e-5)
    assert abs(res_plan[1] - float(acc2[-1])) < 2e-5 * max(1.0, abs(res_plan[1])) and abs(res_plan[2] - int(correct2)) <= 1
    for k, v in res_plan[4].items():
        np.testing.assert_allclose(v.numpy(), m2.state_dict()[k].numpy(), rtol=1e-5, atol=1e-6)
    for k, p in m2.named_parameters():
        if k.endswith("key_projection.bias"):
            continue
        d = np.abs(res_plan[0][k].numpy() - p.detach().numpy())
        assert d.max() <= 3e-4 * 1.01 and (d > 2e-5).mean() <= 2e-3, (k, float(d.max()), float((d > 2e-5).mean()))
