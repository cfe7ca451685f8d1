"""One way to build and run an engine for (precision mode, options, audit stage mask, JEGAL parts mask): what tools/precision_floor.py
prints per round and tests/test_gpu_precision_budget.py asserts are measured on handles set up the same way.

Options that decide how weights are packed (audit_weights, conv_round_diffuse, and jegal_fp32_ends for symmetry) go in BEFORE the
state_dicts; audit_stages / audit_jegal_parts are per run and need audit_weights."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import jegal_amd._lib as L  # noqa: E402
from jegal_amd.gestsync import GestSync  # noqa: E402
from jegal_amd.jegal import JEGAL  # noqa: E402


def open_engine(precision, gsd, jsd, audit_weights=False, opts=()):
    """-> Engine in `precision` with GestSync (gsd) and JEGAL (jsd) loaded; opts: (name, value) pairs or a dict, set before the weights
    are finalized.  audit_weights: keep the fp32 matrices, so that run() can move stages to the fp32 kernels.  The caller closes it."""
    e = L.Engine(0, precision=precision)
    try:
        if audit_weights:
            e.set_option("audit_weights", 1)
        for k, v in (opts.items() if isinstance(opts, dict) else opts):
            e.set_option(k, v)
        GestSync(engine=e).load_state_dict(gsd)
        JEGAL(engine=e).load_state_dict(jsd)
    except BaseException:
        e.close()
        raise
    return e


def run(e, frames_dev, stages=None, jegal_parts=0):
    """-> (gesture embeddings (B, T, 512), GestSync features (B, T, 1024)) as numpy.  stages: audit_stages mask (1 conv stack, 2 GestSync
    transformer + ff_vid, 4 JEGAL gesture branch on the fp32 kernels) and jegal_parts: audit_jegal_parts, both set for this run and left
    set; None: the handle kept no fp32 matrices, nothing is set."""
    if stages is not None:
        e.set_option("audit_stages", stages)
        e.set_option("audit_jegal_parts", jegal_parts)
    emb = e.extract_gesture(frames_dev).cpu().numpy()
    feats = e.gestsync_clip(frames_dev).cpu().numpy()
    return emb, feats
