"""Fixtures of tests/test_gpu_recogniser_kernels.py, built on the CPU: the operands of every recurrent / decoder case with their float64
reference and the same formula in float32 (tests/ref64.py), cached, plus the properties the cases are chosen for, asserted on the float64
reference when a case is built -- the gate spread of every recurrent case, the span of the PEAKED attention rows, "some but not all beams
end".  tests/test_recogniser_cases.py builds every case without a GPU.

Scale.  Inputs and states are uniform in [-1, 1], recurrent weights uniform within 1 / sqrt(K), the gate pre-activations that come from
outside the recurrence (gx of the BiLSTM, the embedding tables E of the two GRU decoders) uniform in [-4, 4]: sigmoid(+-2.94) = 0.95 /
0.05, so about an eighth of the gates sit in either saturated tail whatever the recurrent term (|.| < 1) adds."""
import functools
import math

import torch

import ref64
from dpmn_amd.utils import synth

F32 = torch.float32
SEED = 150


def u(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform("rk_" + name, shape, lo, hi, SEED)


def gate_spread(test, gates):
    """>= 5 % of the sigmoid gate activations below 0.05, >= 5 % above 0.95, >= 20 % in between"""
    g = torch.cat([x.reshape(-1) for x in gates])
    lo, hi = float((g < 0.05).double().mean()), float((g > 0.95).double().mean())
    assert lo >= 0.05 and hi >= 0.05 and 1.0 - lo - hi >= 0.20, "%s: gates %.3f below 0.05, %.3f above 0.95, %.3f between" % (test, lo, hi, 1.0 - lo - hi)
    return lo, hi


# ------------------------------------------------------------------------------------------------------------------ BiLSTM
BILSTM_B, BILSTM_T = (1, 15, 16, 17, 33), (1, 2, 3, 26)


@functools.lru_cache(maxsize=None)
def bilstm_case(B, T):
    gx, whh = u("gx", (B * T, 2048), -4.0, 4.0), u("whh", (2, 1024, 256), -1.0 / 16, 1.0 / 16)
    gates = []
    ref = ref64.bilstm(gx, whh, B, T, gates=gates)
    gate_spread("bilstm[B%d T%d]" % (B, T), gates)
    return gx, whh, ref, ref64.bilstm(gx, whh, B, T, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------ ASTER decoder
ASTER_R, ASTER_T, ASTER_NC = (1, 15, 16, 17, 33), (1, 2, 25, 63, 64), (1, 5, 97, 127, 128)


@functools.lru_cache(maxsize=None)
def aster_weights():
    """every class count takes a prefix: E[:n_class + 1] (row n_class = BOS), fc_w[:n_class], fc_b[:n_class]"""
    k = 1.0 / math.sqrt(512.0)
    return {"s_w": u("a_s_w", (512, 512), -k, k), "s_b": u("a_s_b", (512,), -0.5, 0.5), "w_w": u("a_w_w", (512,), -0.25, 0.25),
            "w_b": u("a_w_b", (1,)), "E": u("a_E", (129, 1536), -4.0, 4.0), "wih_ctx": u("a_wih", (1536, 512), -k, k),
            "whh": u("a_whh", (1536, 512), -k, k), "bhh": u("a_bhh", (1536,), -0.5, 0.5), "fc_w": u("a_fc_w", (128, 512), -4 * k, 4 * k),
            "fc_b": u("a_fc_b", (128,))}


def aster_weights_for(n_class, **replace):
    w = dict(aster_weights(), **replace)
    w["E"], w["fc_w"], w["fc_b"] = w["E"][:n_class + 1].contiguous(), w["fc_w"][:n_class].contiguous(), w["fc_b"][:n_class].contiguous()
    return w


def aster_step_grid():
    """every (R, T) pair; the class counts as a Latin square over it, so every (R, n_class) and (T, n_class) pair occurs once as well"""
    return [(R, T, ASTER_NC[(i + j) % 5]) for i, R in enumerate(ASTER_R) for j, T in enumerate(ASTER_T)]


@functools.lru_cache(maxsize=None)
def aster_step_case(R, T, n_class, peaked=False):
    """-> (w, feats, xproj, row_img, state, y_prev, ref, ref32).  row_img: unsorted, with repeats, image 0 and the last image; y_prev:
    class 0 and the last row of E (BOS) among the rows"""
    w = aster_weights_for(n_class)
    B = 1 if R == 1 else 3
    row_img = torch.tensor(([B - 1, 0] + [(7 * i + 1) % B for i in range(R)])[:R], dtype=torch.int32)
    y_prev = torch.tensor(([n_class, 0] + [(5 * i + 3) % (n_class + 1) for i in range(R)])[:R], dtype=torch.int32)
    feats, xproj, state = u("a_feats", (B, T, 512)), u("a_xproj", (B, T, 512)), u("a_state", (R, 512))
    if peaked:
        # along sign(w_w) every channel pushes the score the same way: -0.32 .. -0.02 at the positions before the last, +0.3 at the last
        a = -0.32 + 0.3 * u("a_peak", (B, T, 1), 0.0, 1.0)
        a[:, -1] = 0.3
        xproj = torch.sign(w["w_w"]) * a + 0.05 * xproj
    gates = []
    ref = ref64.aster_decode_step(w, feats, xproj, row_img, state, y_prev, n_class, gates=gates)
    test = "aster_decode_step[R%d T%d nc%d%s]" % (R, T, n_class, " peaked" if peaked else "")
    gate_spread(test, gates)
    if peaked:
        e = ref["e"]
        span = e.amax(-1) - e.amin(-1)
        assert bool((e.argmax(-1) == T - 1).all()) and 25.0 <= float(span.min()) and float(span.max()) <= 40.0, "%s: span %.1f .. %.1f" % (test, float(span.min()), float(span.max()))
    return w, feats, xproj, row_img, state, y_prev, ref, ref64.aster_decode_step(w, feats, xproj, row_img, state, y_prev, n_class, dtype=F32)


BEAM_SHAPES = ((1, 1), (3, 5), (4, 5), (2, 8), (3, 8))       # R = 1, 15, 20, 16, 24
BEAM_T = (1, 25, 64)
TIE_LEVELS = ((0.0, (3, 70, -1)), (-1.0, (10, 90)), (-2.5, (5, 64, 65, 80)))      # class -1: the last one


def beam_grid():
    """(B, beam, n_class, T, steps): every shape with n_class = beam, 97 and 128 (beam 8 x 128 classes: 1024 candidates, two passes of the
    512 threads); T and steps in turn"""
    out = []
    for i, (B, beam) in enumerate(BEAM_SHAPES):
        for j, n_class in enumerate((beam, 97, 128)):
            out.append((B, beam, n_class, BEAM_T[(i + j) % 3], (1, 6)[(i + j) % 2]))
    return out


def tie_bias(n_class):
    """a classifier bias of a few exactly equal levels (the classifier WEIGHT of the tie case is zero): top level on classes 3, 70 and
    the last one -- both sides of 64 -- then two and four classes; everything else far below, EOS (class 1) lowest"""
    b = -8.0 - 0.25 * (torch.arange(n_class) % 7).float()
    for level, classes in TIE_LEVELS:
        for c in classes:
            b[c % n_class] = level
    b[1] = -20.0
    return b


def tie_expected(beam, n_class):
    """the (beam row, class) choices of steps 0 and 1 of the tie case, best first.  Step 0: only beam row 0 is live, its candidates are
    the bias minus one log-sum-exp: ordered by level, equal levels by class.  Step 1: sequence score + the same log-probabilities, a sum
    of TWO of them -- a + b and b + a are the same bits in any precision, and the top level alone supplies 3 x 3 = 9 >= beam tied
    candidates, so the choices are the first `beam` flat indices among (beam rows holding a top-level class) x (top-level classes)."""
    b = tie_bias(n_class).tolist()
    order = sorted(range(n_class), key=lambda c: (-b[c], c))[:beam]
    top = [c for c in range(n_class) if b[c] == 0.0]
    rows = [k for k, c in enumerate(order) if b[c] == 0.0]
    step1 = sorted((k, c) for k in rows for c in top)[:beam]
    return [(0, c) for c in order], step1


@functools.lru_cache(maxsize=None)
def beam_case(B, beam, n_class, T, kind="cont"):
    """-> (w, feats, xproj, eos).  kind 'eos': the EOS bias raised so that beams end early; 'tie': zero classifier weight, tie_bias"""
    eos = 1 if n_class > 1 else 0
    w = aster_weights_for(n_class)
    if kind == "eos":
        w["fc_b"] = w["fc_b"].clone()
        w["fc_b"][eos] += 3.0
    if kind == "tie":
        w["fc_w"], w["fc_b"] = torch.zeros_like(w["fc_w"]), tie_bias(n_class)
    return w, u("b_feats", (B, T, 512)), u("b_xproj", (B, T, 512)), eos


def some_but_not_all_ended(res, B, beam):
    """an image in which, at some step, at least one beam ended (emitted EOS) and at least one did not"""
    for ended in res["ended"]:
        n = ended.reshape(B, beam).sum(1)
        if bool(((n > 0) & (n < beam)).any()):
            return True
    return False


# ------------------------------------------------------------------------------------------------------------------ MORAN decoder
MORAN_B, MORAN_T, MORAN_NC, MORAN_STEPS = (1, 15, 16, 17, 33), (1, 2, 25, 63, 64), (1, 15, 16, 17, 33, 37, 47, 48), (1, 3, 20)


def moran_grid():
    """every (B, T) pair; class counts and step counts in turn, so each of the 8 class counts meets 3 or 4 different (B, T)"""
    return [(B, T, MORAN_NC[(5 * i + j) % 8], MORAN_STEPS[(i + 2 * j) % 3]) for i, B in enumerate(MORAN_B) for j, T in enumerate(MORAN_T)]


@functools.lru_cache(maxsize=None)
def moran_weights():
    k = 1.0 / 16
    return {"h2h_w": u("m_h2h", (256, 256), -k, k), "h2h_b": u("m_h2hb", (256,), -0.5, 0.5), "score_w": u("m_score", (256,), -0.25, 0.25),
            "E": u("m_E", (49, 768), -4.0, 4.0), "wih_ctx": u("m_wih", (768, 256), -k, k), "whh": u("m_whh", (768, 256), -k, k),
            "bhh": u("m_bhh", (768,), -0.5, 0.5), "gen_w": u("m_gen", (48, 256), -4 * k, 4 * k), "gen_b": u("m_genb", (48,))}


def moran_weights_for(n_class):
    w = dict(moran_weights())
    w["E"], w["gen_w"], w["gen_b"] = w["E"][:n_class + 1].contiguous(), w["gen_w"][:n_class].contiguous(), w["gen_b"][:n_class].contiguous()
    return w


@functools.lru_cache(maxsize=None)
def moran_case(B, T):
    return u("m_feats", (B, T, 256)), u("m_fproj", (B, T, 256))


@functools.lru_cache(maxsize=None)
def moran_free(B, T, n_class, steps):
    """the free-running float64 decoder of a case, with its gate spread asserted -> (logits, ids)"""
    feats, fproj = moran_case(B, T)
    gates = []
    res = ref64.moran_decode(moran_weights_for(n_class), feats, fproj, steps, n_class, gates=gates)
    gate_spread("moran_decode[B%d T%d nc%d steps %d]" % (B, T, n_class, steps), gates)
    return res
