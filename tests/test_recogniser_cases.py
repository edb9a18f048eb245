"""The fixtures of tests/test_gpu_recogniser_kernels.py (tests/recogniser_cases.py) hold what they are chosen for, checked on their float64
references without a GPU: the gate spread of every recurrent case, the PEAKED spans, "some but not all beams end", the tie fixture's
expected choices, and the replay references (which take a kernel's decisions) against the free-running float64 decoders."""
import pytest
import torch

import recogniser_cases as rc
import ref64


@pytest.mark.parametrize("B", rc.BILSTM_B)
def test_bilstm_cases_gate_spread(B):
    for T in rc.BILSTM_T:
        rc.bilstm_case(B, T)          # asserts


@pytest.mark.parametrize("R", rc.ASTER_R)
def test_aster_step_cases_gate_spread(R):
    for r, T, n_class in rc.aster_step_grid():
        if r == R:
            rc.aster_step_case(R, T, n_class)


@pytest.mark.parametrize("T", [25, 64])
def test_aster_step_peaked_span(T):
    rc.aster_step_case(17, T, 97, True)          # asserts: maximum on the last position, span about 30


@pytest.mark.parametrize("B", rc.MORAN_B)
def test_moran_cases_gate_spread_and_replay(B):
    for b, T, n_class, steps in rc.moran_grid():
        if b != B:
            continue
        logits, ids = rc.moran_free(B, T, n_class, steps)
        feats, fproj = rc.moran_case(B, T)
        again, ids2 = ref64.moran_decode(rc.moran_weights_for(n_class), feats, fproj, steps, n_class, ids=ids)
        assert torch.equal(again, logits) and torch.equal(ids2, ids)


def test_moran_wide_margin_case_replays_in_float32():
    """a case whose float64 arg-max margins are far above fp32 round-off: the float32 evaluation that is GIVEN the float64 ids
    reproduces them by its own arg-max as well"""
    B, T, n_class, steps = 3, 25, 5, 6
    logits, ids = rc.moran_free(B, T, n_class, steps)
    top2 = logits.topk(2, -1)[0]
    assert float((top2[..., 0] - top2[..., 1]).min()) > 1e-3
    feats, fproj = rc.moran_case(B, T)
    l32, _ = ref64.moran_decode(rc.moran_weights_for(n_class), feats, fproj, steps, n_class, ids=ids, dtype=torch.float32)
    assert torch.equal(ref64.first_argmax(l32), ids) and float((l32.double() - logits).abs().max()) < 1e-4


def test_beam_replay_is_the_free_running_decoder():
    B, beam, n_class, T, steps = 3, 5, 97, 25, 6
    w, feats, xproj, eos = rc.beam_case(B, beam, n_class, T)
    gates = []
    free = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, gates=gates)
    rc.gate_spread("beam", gates)
    again = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, decisions=(free["sym"], free["pred"]))
    for k in ("score", "state", "seq"):
        assert torch.equal(again[k], free[k]), k
    # at step 0 only beam row 0 of every image is live
    assert bool((free["pred"][0].reshape(B, beam) == torch.arange(B)[:, None] * beam).all())
    r32 = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, decisions=(free["sym"], free["pred"]), dtype=torch.float32)
    assert float((r32["score"].double() - free["score"]).abs().max()) < 1e-4


@pytest.mark.parametrize("B,beam,n_class", [(3, 5, 97), (3, 8, 128), (4, 5, 5)])
def test_beam_eos_case_some_but_not_all_beams_end(B, beam, n_class):
    w, feats, xproj, eos = rc.beam_case(B, beam, n_class, 25, "eos")
    res = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, 6)
    assert rc.some_but_not_all_ended(res, B, beam)
    assert not bool(torch.isnan(res["score"]).any())
    # no child of an ended beam is chosen while a finite candidate remains
    for s in range(6):
        n_finite = torch.isfinite(res["cand"][s]).reshape(B, -1).sum(1).clamp(max=beam)
        assert torch.equal(torch.isfinite(res["score"][s]).reshape(B, beam).sum(1), n_finite)


@pytest.mark.parametrize("beam,n_class", [(5, 97), (8, 97), (8, 128)])
def test_beam_tie_case_expected_choices(beam, n_class):
    """the float64 free-running decoder makes the choices that tie_expected derives by hand from the levels"""
    B = 2
    w, feats, xproj, eos = rc.beam_case(B, beam, n_class, 25, "tie")
    res = ref64.aster_beam(w, feats, xproj, beam, n_class, eos, 2)
    for s, exp in enumerate(rc.tie_expected(beam, n_class)):
        for b in range(B):
            got = [(int(p) - b * beam, int(c)) for p, c in zip(res["pred"][s].reshape(B, beam)[b], res["sym"][s].reshape(B, beam)[b])]
            assert got == exp, "step %d image %d: %s, expected %s" % (s, b, got, exp)
    top = [c for c, v in enumerate(rc.tie_bias(n_class).tolist()) if v == 0.0]
    assert min(top) < 64 < max(top) and len(top) == 3


def test_beam_grid_gate_spread():
    for B, beam, n_class, T, steps in rc.beam_grid():
        w, feats, xproj, eos = rc.beam_case(B, beam, n_class, T)
        gates = []
        ref64.aster_beam(w, feats, xproj, beam, n_class, eos, steps, gates=gates)
        rc.gate_spread("aster_beam[B%d beam%d nc%d T%d steps %d]" % (B, beam, n_class, T, steps), gates)
