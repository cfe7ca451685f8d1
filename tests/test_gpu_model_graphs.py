"""The model graphs (jegal.hip, gestsync.hip, xlmr.hip) are written once and instantiated per arithmetic: 16-bit activations, fp32 on the
fp32 MFMA (audit) and fp32 on the split-operand kernel (the ends).  What holds them together, through the C ABI: audit_jegal_parts = 15
IS the audit stage, each single part moves the output towards it, and every graph issues the launches it issued before it was
templated (tests/golden/model_graph_launches.json, recorded by tools/model_graph_digest.py from the library before that change)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from jegal_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_graph_digest as MG

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "model_graph_launches.json")))


@pytest.fixture(scope="module")
def rc_aw():
    """A default-mode (JG_PREC_FP16_RC) handle that kept the fp32 matrices, JEGAL weights only"""
    from jegal_amd._lib import Engine, PREC_FP16_RC
    from jegal_amd.jegal import JEGAL
    e = Engine(0, precision=PREC_FP16_RC)
    e.set_option("audit_weights", 1)
    JEGAL(engine=e).load_state_dict(synth.jegal_state_dict())
    yield e
    e.close()


def gestures(e, B, T, align, **opts):
    for k in ("audit_stages", "audit_jegal_parts"):
        e.set_option(k, opts.get(k, 0))
    feats, mask = MG.gesture_inputs(B, T, ragged=1)
    out = e.jegal_gestures(feats, mask, align=align).cpu().numpy()
    for k in ("audit_stages", "audit_jegal_parts"):
        e.set_option(k, 0)
    return out


def rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("align", (0, 1))
@pytest.mark.parametrize("B,T", MG.GESTURE_SHAPES)
def test_all_four_parts_are_the_audit_stage_bit_for_bit(rc_aw, B, T, align):
    """Input projection, attention sub-layers, feed-forward sub-layers and tail on the fp32 kernels (audit_jegal_parts = 15) are the
    launches of audit_stages = 4: exact by construction."""
    assert np.array_equal(gestures(rc_aw, B, T, align, audit_jegal_parts=15), gestures(rc_aw, B, T, align, audit_stages=4))


@pytest.mark.parametrize("B,T", MG.GESTURE_SHAPES)
def test_each_part_changes_the_bits_and_stays_in_the_contract(rc_aw, B, T):
    """A single part on the fp32 kernels is another computation than the default (its bits differ) of the same function (within the
    project's contract tolerance, 1e-3 rel-L2, of the fp32 output); with the option back at 0 the default bits return."""
    default, fp32 = gestures(rc_aw, B, T, 1), gestures(rc_aw, B, T, 1, audit_stages=4)
    print(f"\nB={B} T={T} default vs fp32: rel-L2 {rel(default, fp32):.2e}", end="")
    for part in (1, 2, 4, 8):
        got = gestures(rc_aw, B, T, 1, audit_jegal_parts=part)
        print(f" | part {part}: {rel(got, fp32):.2e}", end="")
        assert not np.array_equal(got, default), part
        assert rel(got, fp32) < 1e-3, (part, rel(got, fp32))
        assert np.array_equal(gestures(rc_aw, B, T, 1), default), part


@pytest.mark.parametrize("config", list(MG.CONFIGS))
def test_launches_per_stage_are_those_recorded_before_the_graphs_were_templated(config):
    """Per case of tools/model_graph_digest.py: the launches per profiling stage.  Catches what the outputs can hide -- a LayerNorm with
    two outputs turning into two launches, a dropped zero-tail of rows the caller strips."""
    recs = MG.run_config(config)
    assert recs and all(r["case"] in GOLDEN for r in recs), [r["case"] for r in recs if r["case"] not in GOLDEN]
    assert len(recs) == sum(c.startswith(config + "/") for c in GOLDEN)
    wrong = {r["case"]: (r["launches"], GOLDEN[r["case"]]) for r in recs if r["launches"] != GOLDEN[r["case"]]}
    assert not wrong, wrong
