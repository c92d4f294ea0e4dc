"""The scaffold the matchers and the place database share, no GPU: the host half (csrc/call_layout.h, place_layout.h) under the
sanitizers as a stand-alone program, the shape of the sources that use the shared headers, and the binding's one helper behind the
matchers' buffers and one timed handle behind the image front end."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from slslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "slslam_amd", "csrc")


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def test_host_half_under_the_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "call_block_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "call_block_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "call block ok" in r.stdout


def test_the_matchers_share_one_core_and_one_scaffold():
    """One finish kernel, one key and one running best (mutual_match.h); one device check (call_block.h); no layout of a matcher written
    as a chain of sums."""
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))}
    for name, text in sources.items():
        assert "k_match_finish" not in text and "k_desc_finish" not in text, name
    for name in ("line_match.h", "descriptor_match.h"):
        assert "atomicMin(" not in sources[name] and "__shfl_xor(" not in sources[name], name
        assert '#include "mutual_match.h"' in sources[name] and "offer_key(" in sources[name] and "take_pair(" in sources[name], name
    shared = sources["mutual_match.h"]
    assert shared.count("atomicMin(") == 1 and shared.count("__shfl_xor(") == 1 and shared.count("__global__") == 1
    users = {name: text.count("hipGetDeviceCount") for name, text in sources.items() if "hipGetDeviceCount" in text}
    assert users == {"call_block.h": 1, "lba_api.hip": 1}, users
    lba = sources["lba_api.hip"]
    body = lba[lba.index('extern "C" int slslam_device_count'):]
    assert "hipGetDeviceCount" in body[:body.index("\n}\n")]
    for name in ("match_api.hip", "descriptor_api.hip"):
        assert '#include "call_block.h"' in sources[name] and not re.search(r"struct\s+Layout\b", sources[name]), name
        assert "match_bind(" in sources[name] and "match_clear(" in sources[name] and "match_download(" in sources[name], name
        assert "match_scatter(" in sources[name] and "std::memcpy(r." not in sources[name], name
    for name in ("match_api.hip", "descriptor_api.hip", "place_api.hip", "place_layout.h", "voctree_train_api.hip"):
        assert not re.search(r"=\s*y\.\w+\s*\+\s*align256\(", sources[name]), name


def test_the_front_end_shares_one_pair_kernel_and_one_timed_handle():
    """One gated pair kernel and one set of its constants (gated_pairs.h, call_layout.h); one pair of events, one grid limit
    (call_block.h)."""
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))}
    assert [name for name, text in sources.items() if re.search(r"\bkQueryStride\s*=", text)] == ["gated_pairs.h"]
    for name, text in sources.items():
        assert not re.search(r"__global__[^;{]*\bk_(stereo|track)_pairs\b", text), name
    for name in ("stereo_match.h", "line_track.h"):
        assert '#include "gated_pairs.h"' in sources[name] and "__global__ __launch_bounds__(64) void k_gated_pairs" not in sources[name], name
        assert "__ffsll(" not in sources[name], name
    assert sources["gated_pairs.h"].count("__global__") == 1 and "#pragma STDC FP_CONTRACT OFF" in sources["gated_pairs.h"]
    for name in ("stereo_api.hip", "track_api.hip"):
        assert "k_gated_pairs<Pairs>" in sources[name], name
    for name in ("descriptor_match.h", "gated_pairs.h"):
        assert "stage_rows(" in sources[name] and "group_chains(" in sources[name], name
    for name in ("line_detect_api.hip", "line_descriptor_api.hip", "stereo_api.hip", "track_api.hip"):
        assert "hipEvent" not in sources[name] and "TimedHandle" in sources[name] and "handle_timing(" in sources[name], name
    for name in ("line_detect_api.hip", "line_descriptor_api.hip", "stereo_api.hip", "track_api.hip", "match_api.hip", "descriptor_api.hip"):
        assert "65535" not in sources[name], name
    assert sources["call_block.h"].count("65535") == 1
    assert sum(text.count("inline int segment_ok(") for text in sources.values()) == 1
    assert sum(text.count("inline bool shape_valid(") for text in sources.values()) == 1


def test_one_timed_handle_and_one_options_helper_in_the_binding():
    image = np.zeros((32, 32), dtype=np.uint8)
    for make, sym in ((capi.LineDescriptor, "slslam_line_descriptor"), (capi.LineDetector, "slslam_line_detector"),
                      (lambda: capi.StereoMatcher(8), "slslam_stereo_matcher"), (lambda: capi.LineTracker(8), "slslam_line_tracker")):
        h = make()
        assert isinstance(h, capi._TimedHandle), sym
        assert (h._DESTROY, h._STATS, h._TIMING) == (sym + "_destroy", sym + "_stats", sym + "_timing")
        assert "set_timing" not in vars(type(h)) and "kernel_ms" not in vars(type(h)), sym
        assert h.kernel_ms() == 0.0
        h.set_timing(True)
        h.set_timing(False)
        assert h.kernel_ms() == 0.0
        h.close()
        h.close()
    with pytest.raises(TypeError, match=r"^unknown stereo match option 'nope'$"):
        capi.stereo_match_options(nope=1)
    with pytest.raises(TypeError, match=r"^unknown line track option 'nope'$"):
        capi.line_track_options(nope=1)
    assert capi.stereo_match_options(max_disparity=64).max_disparity == 64.0 and capi.line_track_options(max_shift=3).max_shift == 3.0
    with pytest.raises(ValueError, match=r"^an image is uint8 \[H, W\]$"):
        capi.describe_lines(image.astype(np.float32), np.zeros((1, 4), dtype=np.float32))
    with pytest.raises(ValueError, match=r"^an image is uint8 \[H, W\]$"):
        capi.detect_lines(np.zeros((4, 4, 3), dtype=np.uint8))


def test_one_buffers_helper_behind_both_matchers():
    for make, result, keys, lens in (
            (capi._match_buffers, capi.MatchResult, ("match", "best_line", "best_error", "second_error", "num_admissible", "best_observation"), (3, 5)),
            (capi._desc_buffers, capi.DescriptorResult, ("match", "best", "best_distance", "second_distance", "num_admissible", "best_query"), (0, 2))):
        n, m = lens
        r, b = make(n, m)
        assert isinstance(r, result) and tuple(b) == keys and r.status == -1 and r.num_matched == 0
        for i, k in enumerate(keys):
            want = np.float32 if i in (2, 3) else np.int32
            assert b[k].dtype == want and len(b[k]) == max(m if i == 5 else n, 1), k
            assert (b[k] == (0 if i in (2, 3, 4) else -2)).all(), k
            assert C.addressof(getattr(r, k).contents) == b[k].ctypes.data, k
    r, b = capi._match_buffers(3, 5)
    r.status, r.num_matched = 0, 2
    out = capi._match_dict(r, b, 3, 5)
    assert list(out) == ["status", "num_matched", "match", "best_line", "best_error", "second_error", "num_admissible", "best_observation"]
    assert out["status"] == "OK" and out["num_matched"] == 2 and len(out["match"]) == 3 and len(out["best_observation"]) == 5
    r, b = capi._desc_buffers(4, 6)
    r.status, r.num_keyframe_descriptors = 0, 6
    out = capi._desc_dict(r, b, 4, 7)
    assert list(out)[:3] == ["status", "num_matched", "candidate"] and out["candidate"] == 7
    assert len(out["best"]) == 4 and len(out["best_query"]) == 6
