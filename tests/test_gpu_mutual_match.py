"""GPU test: what the line matcher and the descriptor matcher share (csrc/mutual_match.h: the key, the running best and
k_mutual_finish; csrc/call_block.h: the handle and its blocks) with one handle of each alive in the same process and used in turn, at
the edges of a wave and of a group of eight.  Each result equals its numpy reference bit for bit, and the bytes a fresh handle gives."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as R  # noqa: E402
import line_match_reference as M  # noqa: E402
import test_gpu_descriptor_match as TD  # noqa: E402
import test_gpu_line_match as TL  # noqa: E402

pytestmark = pytest.mark.gpu

D, RATIO, MAX_DISTANCE, MARGIN = 72, 1.2, 0.9, 0.05


def test_two_matchers_in_turn(hip):
    frames = [M.make_frame(7000 + 10 * K + L, K, L, extents=True) for K in (1, 65) for L in (63, 65)]
    line_ref = [M.match(fr, margin=MARGIN) for fr in frames]
    for r in line_ref:
        TL.clear_of_boundary(r)
    queries, keyframes = TD.make_views(172, [1, 65], [7, 9, 65], D)
    store = R.Store()
    for k in keyframes:
        store.insert(k)
    call = [(q, [0, 1, 2]) for q in queries]
    desc_ref = store.run(call, RATIO, MAX_DISTANCE)
    assert max(r["num_matched"] for r in line_ref) > 30 and desc_ref[1][2]["num_matched"] > 30     # (the cases are not empty ones)

    def descriptor_matcher():
        m = hip.DescriptorMatcher(D, max_keyframes=3, max_descriptors=65, max_frames=2, max_candidates=3)
        for k in keyframes:
            assert m.insert(k)["status"] == "OK"
        return m

    lm, dm = hip.LineMatcher(max_frames=4, max_observations=65, max_lines=65), descriptor_matcher()
    line_got = desc_got = None
    for turn in range(2):
        # one problem, then all of them: each matcher's block holds the other call's sizes of its own kind in between
        i, j = turn, 1 - turn
        TL.same(lm.run(frames[i:i + 1], margin=MARGIN)[0], line_ref[i])
        for g, r in zip(dm.run(call[j:j + 1], RATIO, MAX_DISTANCE)[0], desc_ref[j]):
            TD.same(g, r)
        line_got = lm.run(frames, margin=MARGIN)
        desc_got = dm.run(call, RATIO, MAX_DISTANCE)
        for g, r in zip(line_got, line_ref):
            TL.same(g, r)
        for gf, rf in zip(desc_got, desc_ref):
            for g, r in zip(gf, rf):
                TD.same(g, r)
    assert lm.stats() == {"calls": 4, "allocations": 1} and dm.stats() == {"calls": 3 + 4, "allocations": 2}

    fresh_l, fresh_d = hip.LineMatcher(max_frames=4, max_observations=65, max_lines=65), descriptor_matcher()
    for g, f in zip(line_got, fresh_l.run(frames, margin=MARGIN)):
        TL.same_bytes(g, f)
    for gf, ff in zip(desc_got, fresh_d.run(call, RATIO, MAX_DISTANCE)):
        for g, f in zip(gf, ff):
            TD.same_bytes(g, f)
    for m in (lm, dm, fresh_l, fresh_d):
        m.close()
