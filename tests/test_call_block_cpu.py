"""The scaffold the matchers and the place database share, no GPU: the host half (csrc/call_layout.h, place_layout.h) under the
sanitizers as a stand-alone program, the shape of the sources that use the shared headers, and the binding's one helper behind the
matchers' buffers."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np

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
