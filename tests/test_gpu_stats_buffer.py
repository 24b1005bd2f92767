"""The one work buffer of the statistics launches on the MI355X (dr_engine::stats_work): "cfg_rescale" and "cfg_project" /
"cfg_norm" point their launches into the same words, so on ONE engine the probes (dr_debug_project / dr_debug_rescale) and
the captured chains of the two options alternate - every result bit-equal to the CPU restatement (tests/project_ref.py,
tests/rescale_ref.py) and to its own earlier run: neither launch leaves the other anything it reads (the ticket is zero
between launches, every slot a launch adds up is its own), and a switch costs the other option's chain nothing."""
import numpy as np
import pytest
import torch

from testlib import make_model, same_bits

import project_ref as PR
import rescale_cases as RC
import rescale_ref as RR
import thresh_ref as TR

pytestmark = pytest.mark.gpu

W = 3.0
PROJECT, NORM, PHI = 5000, 500, 7000


# (B, T, window_overlap, window_blend): the one-workgroup form, the first roll of the grid form, the grid form over a canvas
@pytest.mark.parametrize("B,T,O,mode", [(2, 40, 0, 0), (2, 745, 0, 0), (3, 32, 5, 1)], ids=["roll-form", "grid-form", "window-canvas"])
def test_probes_alternate_on_one_engine(B, T, O, mode):
    g = torch.Generator().manual_seed(T)
    c, u = 1.2 * torch.randn(B, T, 88, generator=g) + 0.5, torch.randn(B, T, 88, generator=g)
    groups, plan = (TR.window_groups(B, O), (O, mode)) if O else (TR.clip_groups(B), None)
    want_ab = PR.group_ab(c, u, W, PROJECT, NORM, groups, plan)
    want_g = RR.group_g(c, u, W, PHI, groups, plan)
    print(f"\nstats buffer B {B} T {T} O {O}: g {want_g.tolist()} (a, b) {want_ab.tolist()}")
    # neither result is an identity: a buffer that handed one launch the other's words would show
    assert (np.abs(want_g - 1.0) >= 0.5).all() and (want_ab[:, 0] >= 0.9).all() and (want_ab[:, 1] <= 0.05).all(), (want_g, want_ab)
    hp, p, _, _, _ = RC.setup()
    eng = make_model(hp, p, sampler="cfdg_ddpm_x0").engine

    def project():
        eng.set_option("cfg_rescale", 0)
        eng.set_option("cfg_project", PROJECT)
        eng.set_option("cfg_norm", NORM)
        return eng.project_stats(c, u, W, groups=len(groups))

    def rescale():
        eng.set_option("cfg_project", 0)
        eng.set_option("cfg_norm", 0)
        eng.set_option("cfg_rescale", PHI)
        return eng.rescale_stats(c, u, W, groups=len(groups))

    try:
        eng.set_option("window_overlap", O)
        eng.set_option("window_blend", mode)
        ab, gg, ab2, gg2 = project(), rescale(), project(), rescale()
    finally:
        for name in ("cfg_rescale", "cfg_project", "cfg_norm", "window_blend", "window_overlap"):
            eng.set_option(name, 0)
    assert same_bits(ab, torch.from_numpy(want_ab)), (ab.cpu().tolist(), want_ab.tolist())
    assert same_bits(gg, torch.from_numpy(want_g)), (gg.cpu().tolist(), want_g.tolist())
    assert same_bits(ab2, ab) and same_bits(gg2, gg)


def test_chains_alternate_on_one_engine():
    """4 visited steps, Philox noise: the captured chain of "cfg_rescale", that of "cfg_project", the first again."""
    hp, p, wav, x, _ = RC.setup()
    eng = make_model(hp, p, sampler="cfdg_ddpm_x0", w=RC.W).engine
    eng.frontend(wav, RC.TN)
    x_T = x.squeeze(1).to(eng.device).contiguous()

    def run(name, value, other, **kw):
        eng.set_option(other, 0)
        eng.set_option(name, value)
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=RC.W, seed=RC.PHILOX_SEED, **kw)

    try:
        eng.set_option("sampling_steps", 4)
        first = run("cfg_rescale", 7000, "cfg_project")
        second = run("cfg_project", 10000, "cfg_rescale")
        third = run("cfg_rescale", 7000, "cfg_project")
        eager_rescale = run("cfg_rescale", 7000, "cfg_project", use_graph=False)
        eager_project = run("cfg_project", 10000, "cfg_rescale", use_graph=False)
    finally:
        for name in ("cfg_rescale", "cfg_project", "sampling_steps"):
            eng.set_option(name, 0)
    assert torch.equal(third, first)
    assert torch.equal(first, eager_rescale) and torch.equal(second, eager_project)
    assert not torch.equal(first, second)
