"""The argument rules of Engine's metric entries (jegal_amd/_metric_entries.py) without a GPU: the table of limits equals the constants of
csrc/shared.h, and entry by entry what is refused (ValueError, before the wrapper touches its handle) and what is not: one good call on
tiny inputs per entry, single-argument changes that must be refused -- every limit one step past it, every offsets argument with too few
entries, a negative first entry, a decreasing pair and a last entry beyond the rows -- and the largest legal value of every limit, which must
get past the checks.  CASES is data, so that the same table can be run against another build of the package."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
z = torch.zeros


def _entry(good, bad, ok):
    return dict(good=good, bad=bad, ok=ok)


def _offset_cases(name, short, rows):
    """the four ways in which the offsets [0, a, rows] of `name` can be wrong; `short`: the array with too few entries"""
    return [{name: short}, {name: [-1, 1, rows]}, {name: [0, rows, rows - 1]}, {name: [0, 1, rows + 1]}]


I3 = z(4, 3, dtype=torch.int32)
WS, WE = [0, 5, 0, 5, 10, 15], [3, 8, 3, 8, 13, 18]
CASES = {
    "pool_mean": _entry(
        dict(x=z(9, 64), offsets=[0, 4, 9]),
        _offset_cases("offsets", [], 9) + [dict(x=z(64)), dict(x=z(9, 0))],
        [dict(offsets=[0, 0, 9]), dict(offsets=torch.tensor([0, 4, 9])), dict(x=z(9, 100))]),
    "sim_rank": _entry(
        dict(e1=z(5, 64), e2=z(20, 64), row_offset=3),
        [dict(e1=z(5, 96), e2=z(20, 96)), dict(e2=z(20, 128)), dict(e1=z(5, 0), e2=z(20, 0)), dict(row_offset=-1), dict(row_offset=16)],
        [dict(row_offset=15), dict(e1=z(5, 1088), e2=z(20, 1088))]),
    "sim_topk": _entry(
        dict(queries=z(5, 64), gallery=z(7, 64), k=3),
        [dict(k=0), dict(k=129), dict(queries=z(5, 96), gallery=z(7, 96)), dict(gallery=z(7, 128)), dict(gallery_offset=-1),
         dict(gallery_offset=2 ** 31 - 7)],
        [dict(k=1), dict(k=128), dict(gallery_offset=2 ** 31 - 8), dict(queries=z(5, 1088), gallery=z(7, 1088))]),
    "sim_topk_grouped": _entry(
        dict(queries=z(5, 64), gallery=z(7, 64), g_offsets=[0, 3, 7], k=3),
        [dict(k=0), dict(k=129), dict(queries=z(5, 96), gallery=z(7, 96))] + _offset_cases("g_offsets", [], 7),
        [dict(k=128), dict(g_offsets=[0, 0, 7]), dict(g_offsets=[2, 3, 6]), dict(g_offsets=torch.tensor([0, 3, 7]))]),
    "group_of_rows": _entry(
        dict(idx=I3, g_offsets=[0, 3, 7]),
        [dict(g_offsets=[]), dict(g_offsets=[-1, 3, 7]), dict(g_offsets=[0, 5, 3]), dict(g_offsets=[0, 3, 2 ** 31]), dict(gallery_offset=-1),
         dict(gallery_offset=2 ** 31), dict(idx=I3.to(torch.int64))],
        [dict(gallery_offset=2 ** 31 - 1), dict(g_offsets=[0, 3, 2 ** 31 - 1])]),
    "spot": _entry(
        dict(gesture=z(10, 64), content=z(6, 64), g_offsets=[0, 4, 10], c_offsets=[0, 2, 6], targets=[1, 3]),
        _offset_cases("g_offsets", [0, 10], 10) + _offset_cases("c_offsets", [0, 6], 6)
        + [dict(targets=[2, 3]), dict(targets=[1, 4]), dict(targets=[-1, 0]), dict(content=z(6, 128)),
           dict(content=z(1025, 64), c_offsets=[0, 1025], g_offsets=[0, 10], targets=[0]),                       # 1025 words
           dict(gesture=z(8193, 64), g_offsets=[0, 8193], c_offsets=[0, 6], targets=[0])],                       # 8193 frames
        [dict(content=z(1024, 64), c_offsets=[0, 1024], g_offsets=[0, 10], targets=[1023]),
         dict(gesture=z(8192, 64), g_offsets=[0, 8192], c_offsets=[0, 6], targets=[0]),
         dict(gesture=z(10, 96), content=z(6, 96))]),                                                            # spot_kernel takes any D
    "attn_matrix": _entry(
        dict(gesture=z(10, 64), content=z(6, 64), g_offsets=[0, 4, 10], c_offsets=[0, 2, 6]),
        _offset_cases("g_offsets", [0, 10], 10) + _offset_cases("c_offsets", [0, 6], 6)
        + [dict(gesture=z(10, 96), content=z(6, 96)), dict(gesture=z(10, 0), content=z(6, 0)), dict(content=z(6, 128)), dict(temp=0.0),
           dict(content=z(1025, 64), c_offsets=[0, 1025], g_offsets=[0, 10]), dict(gesture=z(8193, 64), g_offsets=[0, 8193], c_offsets=[0, 6])],
        [dict(content=z(1024, 64), c_offsets=[0, 1024], g_offsets=[0, 10]), dict(gesture=z(8192, 64), g_offsets=[0, 8192], c_offsets=[0, 6]),
         dict(gesture=z(10, 1088), content=z(6, 1088))]),
    "sync_offset": _entry(
        dict(vid=z(10, 64), aud=z(9, 64), v_offsets=[0, 4, 10], a_offsets=[0, 5, 9]),
        _offset_cases("v_offsets", [0, 10], 10) + _offset_cases("a_offsets", [0, 9], 9)
        + [dict(max_shift=65), dict(max_shift=-1), dict(min_overlap=0), dict(vid=z(10, 96), aud=z(9, 96)), dict(vid=z(10, 1088), aud=z(9, 1088)),
           dict(aud=z(9, 128))],
        [dict(max_shift=64), dict(max_shift=0), dict(vid=z(10, 1024), aud=z(9, 1024)), dict(v_offsets=[0, 0, 10]),
         dict(v_offsets=torch.tensor([0, 4, 10]), a_offsets=torch.tensor([0, 5, 9]))]),
    "asd": _entry(
        dict(query=z(2, 64), cand=z(9, 64), c_offsets=[0, 4, 9]),
        _offset_cases("c_offsets", [0, 9], 9) + [dict(cand=z(9, 128)), dict(query=z(64))],
        [dict(c_offsets=[0, 0, 9]), dict(query=z(2, 96), cand=z(9, 96)), dict(c_offsets=torch.tensor([0, 4, 9]))]),
    "asd_windows": _entry(
        dict(gesture=z(30, 64), g_offsets=[0, 10, 30], content=z(6, 64), c_offsets=[0, 2, 6], trk=[0, 1, 1], s_offsets=[0, 2, 3], win=5, hop=2,
             word_start=WS, word_end=WE),
        _offset_cases("g_offsets", [0, 30], 30) + _offset_cases("c_offsets", [0, 6], 6) + _offset_cases("s_offsets", [0, 3], 3)
        + [dict(trk=[0, 2, 1]), dict(trk=[0, -1, 1]), dict(win=8193), dict(win=-1), dict(hop=0), dict(temp=0.0), dict(n_windows=[3, 8193]),
           dict(gesture=z(30, 96), content=z(6, 96)), dict(gesture=z(30, 1088), content=z(6, 1088)), dict(content=z(6, 128)),
           dict(trk=[0] * 65, s_offsets=[0, 65], c_offsets=[0, 6]),                                             # 65 candidates
           dict(content=z(1025, 64), c_offsets=[0, 1025], trk=[0], s_offsets=[0, 1], win=0),                    # 1025 words
           dict(gesture=z(8193, 64), g_offsets=[0, 8193], trk=[0], s_offsets=[0, 1], c_offsets=[0, 6], win=0)], # 8193 frames
        [dict(win=8192), dict(n_windows=[3, 8192]), dict(gesture=z(30, 1024), content=z(6, 1024)),
         dict(trk=[0] * 64, s_offsets=[0, 64], c_offsets=[0, 6]),
         dict(content=z(1024, 64), c_offsets=[0, 1024], trk=[0], s_offsets=[0, 1], win=0),
         dict(gesture=z(8192, 64), g_offsets=[0, 8192], trk=[0], s_offsets=[0, 1], c_offsets=[0, 6], win=0)]),
}


def outcome(engine, entry, kwargs):
    """"refused" (ValueError), "passed" (the checks are behind it: the handle-less engine fails at its first use of the handle) or the
    name of whatever else was raised"""
    try:
        getattr(engine, entry)(**kwargs)
    except ValueError:
        return "refused"
    except AttributeError:
        return "passed"
    except Exception as e:
        return type(e).__name__
    return "returned"


def test_limits_table_equals_the_constants_of_shared_h():
    from jegal_amd._metric_entries import LIMITS
    consts = {}
    text = open(os.path.join(ROOT, "jegal_amd", "csrc", "shared.h")).read()
    for decl in re.findall(r"constexpr int ([^;]+);", text):          # "NAME = value" or several of them, value = n or n << m
        for part in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*", part)
            if m:
                consts[m[1]] = int(m[2]) << int(m[3] or 0)
    assert len(LIMITS) >= 12
    missing = sorted(set(LIMITS) - set(consts))
    assert not missing, f"not declared in shared.h: {missing}"
    assert LIMITS == {k: consts[k] for k in LIMITS}
    assert consts["SYNCW_MAX_T"] == 2 ** 20 and consts["SPOT_MAX_W"] == 1024          # the parser reads both forms


@pytest.mark.parametrize("entry", sorted(CASES))
def test_entry_refuses_what_is_out_of_bounds_and_nothing_else(entry):
    from jegal_amd._lib import Engine
    eng = Engine.__new__(Engine)                     # no handle, no device: every check comes before either is touched
    case = CASES[entry]
    assert outcome(eng, entry, case["good"]) == "passed"
    wrong = [(kw, "refused", got) for kw in case["bad"] if (got := outcome(eng, entry, dict(case["good"], **kw))) != "refused"]
    wrong += [(kw, "passed", got) for kw in case["ok"] if (got := outcome(eng, entry, dict(case["good"], **kw))) != "passed"]
    assert not wrong, [({k: (tuple(v.shape) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}, want, got) for kw, want, got in wrong]
