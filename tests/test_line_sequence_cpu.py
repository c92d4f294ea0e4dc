"""The ends of the tracker's chain without a device: synth.make_line_sequence, the accuracy the numpy tracker
(tests/line_track_reference.py) reaches on it with reference MSLD descriptors, the reference chain detector -> MSLD -> stereo pairing
-> tracking that tests/test_gpu_line_track.py compares capi.detect_describe_pair_and_track with, and the frame-file writer
(host/sequence_io.h: slslam_write_frame_file, slslam_format_frame_text) against the reader."""
import ctypes as C
import functools
import os
import sys

import numpy as np

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_descriptor_reference as MSLD  # noqa: E402
import line_detect_reference as LSD  # noqa: E402
import line_track_reference as R  # noqa: E402
import stereo_match_reference as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "slslam_amd", "_lib", "libslslam_host.so")
KITTI = dict(fx=406.05, fy=406.05, cx=327.783, cy=237.172)

SEQ_SEED, SEQ_FRAMES, SEQ_DISPARITY = 6, 6, 8.0
STEREO_OPTIONS = dict(max_disparity=16.0)
SEQ_TRUE_LINKS = 50              # consecutive-frame pairs of rows that show the same drawn segment
SEQ_LINKS_FOUND = 44             # of them, those the numpy tracker continues: recorded, not chosen (the first seed tried)
CHAIN_LINKS = 38                 # links of the reference chain between detections of the same drawn edge: recorded, not chosen


def shifts():
    """The scene's position in every frame: steps of up to 6 px a frame and axis, from (0, 0)."""
    s = np.cumsum(np.random.default_rng(SEQ_SEED).uniform(-6.0, 6.0, (SEQ_FRAMES, 2)), axis=0)
    return np.clip(s - s[0], -14.0, 14.0)


@functools.lru_cache(maxsize=None)
def sequence():
    return synth.make_line_sequence(SEQ_SEED, 160, 224, 12, SEQ_FRAMES, shifts(), drop=0.15, disparity=SEQ_DISPARITY, max_length=60)


def test_make_line_sequence():
    s, q = sequence(), synth.make_line_sequence(SEQ_SEED, 160, 224, 12, SEQ_FRAMES, shifts(), drop=0.15, disparity=SEQ_DISPARITY, max_length=60)
    for k in s:
        assert len(s[k]) == SEQ_FRAMES and all(np.array_equal(a, b) for a, b in zip(s[k], q[k])), k
    step = np.abs(np.diff(shifts(), axis=0))
    assert 5.0 < step.max() <= 6.0 and (step != np.rint(step)).all()                          # sub-pixel, up to about 6 px
    assert sorted(s["labels"][0].tolist()) == list(range(12)) and s["labels"][0].tolist() != list(range(12))
    assert min(len(x) for x in s["labels"]) < 12                                              # some segments are absent from some frames
    base = {int(k): seg for k, seg in zip(s["labels"][0], s["segments"][0].astype(np.float64))}
    for t in range(SEQ_FRAMES):
        assert s["images"][t].dtype == np.uint8 and s["images"][t].shape == s["right_images"][t].shape == (160, 224)
        assert len(set(s["labels"][t].tolist())) == len(s["labels"][t]) == len(s["segments"][t])
        assert sorted(s["labels"][t].tolist()) == sorted(s["right_labels"][t].tolist())
        moved = np.tile(shifts()[t], 2)
        for k, seg in zip(s["labels"][t], s["segments"][t].astype(np.float64)):                # the scene's segment, moved by the shift
            assert np.abs(seg - base[int(k)] - moved).max() < 1e-4
        right = {int(k): seg for k, seg in zip(s["right_labels"][t], s["right_segments"][t].astype(np.float64))}
        for k, seg in zip(s["labels"][t], s["segments"][t].astype(np.float64)):
            assert np.abs(seg - right[int(k)] - [SEQ_DISPARITY, 0, SEQ_DISPARITY, 0]).max() < 1e-4
        assert min(s["segments"][t].min(), s["right_segments"][t].min()) >= 26.0 - 1e-4
        if t:
            assert not np.array_equal(s["images"][t], s["images"][t - 1])
    # no disparity: no right view, the same left one
    p = synth.make_line_sequence(SEQ_SEED, 160, 224, 12, 2, shifts()[:2], drop=0.0, max_length=60)
    assert set(p) == {"images", "segments", "labels"} and [len(x) for x in p["labels"]] == [12, 12]


def links(labels_prev, labels, match):
    """(true links, those found, wrong links) of one frame against the frame before it."""
    prev = [int(x) for x in labels_prev]
    true = sum(1 for x in labels if x >= 0 and int(x) in prev)
    found = sum(1 for a, m in enumerate(match) if m >= 0 and labels[a] >= 0 and prev[m] == int(labels[a]))
    return true, found, int((np.asarray(match) >= 0).sum()) - found


def test_accuracy_on_the_generators_segments():
    """The drawn segments with reference MSLD descriptors through the numpy tracker: no wrong link, and the recorded share of the
    true ones; every id names one drawn segment for as long as it is seen without a gap."""
    s = sequence()
    frames = []
    for img, seg in zip(s["images"], s["segments"]):
        d = MSLD.describe(img, seg)
        assert set(d["status"]) == {MSLD.OK}
        frames.append((seg, d["descriptors"].astype(np.float32)))
    out = R.track(frames)
    got = np.array([links(s["labels"][t - 1], s["labels"][t], out[t]["match"]) for t in range(1, SEQ_FRAMES)]).sum(axis=0)
    print("generator segments: %d true links, %d found, %d wrong" % tuple(got))
    assert got.tolist() == [SEQ_TRUE_LINKS, SEQ_LINKS_FOUND, 0]
    owner = {}
    for t in range(SEQ_FRAMES):
        for a, i in enumerate(out[t]["id"]):
            assert i >= 0 and owner.setdefault(int(i), int(s["labels"][t][a])) == int(s["labels"][t][a])
    assert sum(o["num_new"] for o in out) == len(owner)


def owner_of(drawn, labels, seg, reach=2.0, beyond=6.0):
    """The label of the drawn segment that the detection `seg` lies on (tests/test_stereo_match_cpu.py words it the same way); -1: none."""
    for lab, s in zip(labels, np.asarray(drawn, dtype=np.float64)):
        length = np.hypot(*(s[2:] - s[:2]))
        d = (s[2:] - s[:2]) / length
        ok = True
        for p in (seg[:2], seg[2:]):
            along = (p[0] - s[0]) * d[0] + (p[1] - s[1]) * d[1]
            across = abs((p[0] - s[0]) * d[1] - (p[1] - s[1]) * d[0])
            ok = ok and across <= reach and -beyond <= along <= length + beyond
        if ok:
            return int(lab)
    return -1


@functools.lru_cache(maxsize=None)
def chain_reference():
    """detector -> MSLD -> stereo pairing -> tracking of the left segments, reference implementations.  Per frame dict(left_rows,
    right_rows, stereo, track, ids, observations, labels: the drawn segment under every tracked row, -1: none)."""
    s = sequence()
    per, frames = [], []
    for t in range(SEQ_FRAMES):
        a, b = LSD.detect(s["images"][t]), LSD.detect(s["right_images"][t])
        da = MSLD.describe(s["images"][t], a["segments"].astype(np.float32))
        db = MSLD.describe(s["right_images"][t], b["segments"].astype(np.float32))
        ka, kb = (np.nonzero(np.array([x == MSLD.OK for x in d["status"]], dtype=bool))[0] for d in (da, db))
        ls, ld = a["segments"][ka].astype(np.float32), da["descriptors"][ka].astype(np.float32).reshape(len(ka), -1)
        m = SR.match(ls, ld, b["segments"][kb].astype(np.float32), db["descriptors"][kb].astype(np.float32).reshape(len(kb), -1),
                     **STEREO_OPTIONS)
        frames.append((ls, ld))
        per.append(dict(left_rows=ka, right_rows=kb, stereo=m,
                        labels=np.array([owner_of(s["segments"][t], s["labels"][t], x) for x in ls.astype(np.float64)], dtype=np.int64)))
    for p, tr in zip(per, R.track(frames)):
        obs, idx = SR.observations(p["stereo"])
        p.update(track=tr, ids=tr["id"][idx], observations=obs, index=idx)
    return per


def test_accuracy_of_the_reference_chain():
    per = chain_reference()
    got = np.array([links(per[t - 1]["labels"], per[t]["labels"], per[t]["track"]["match"]) for t in range(1, SEQ_FRAMES)]).sum(axis=0)
    both = sum(1 for t in range(1, SEQ_FRAMES) for a, m in enumerate(per[t]["track"]["match"])
               if m >= 0 and per[t]["labels"][a] >= 0 and per[t - 1]["labels"][m] >= 0 and per[t]["labels"][a] != per[t - 1]["labels"][m])
    print("reference chain: detections %s, links between detections of the same drawn edge %d, of two different drawn edges %d, all links %d"
          % ([len(p["left_rows"]) for p in per], got[1], both, got[1] + got[2]))
    assert got[1] == CHAIN_LINKS and both == 0
    assert min(len(p["ids"]) for p in per) >= 3                                               # every frame file has lines


# ---- the frame-file writer against the reader
class Intr(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class Frame(C.Structure):
    _fields_ = [("num_lines", C.c_int), ("ids", C.POINTER(C.c_int)), ("observations", C.POINTER(C.c_double))]


@functools.lru_cache(maxsize=None)
def host():
    if not os.path.exists(HOST_LIB):
        import __graft_entry__
        __graft_entry__.build()
    H = C.CDLL(HOST_LIB)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    H.slslam_format_frame_text.argtypes = [C.c_int, ip, dp, C.c_char_p, C.c_size_t]
    H.slslam_format_frame_text.restype = C.c_long
    H.slslam_write_frame_file.argtypes = [C.c_char_p, C.c_int, ip, dp]
    H.slslam_parse_frame_text.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Intr), ip, ip, C.c_int, C.POINTER(Frame)]
    H.slslam_read_frame_file.argtypes = [C.c_char_p, C.POINTER(Intr), ip, ip, C.c_int, C.POINTER(Frame)]
    return H


def frame_text(ids, obs_px):
    H = host()
    ids, obs_px = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(obs_px, dtype=np.float64).reshape(-1, 8)
    ip, dp = ids.ctypes.data_as(C.POINTER(C.c_int)), obs_px.ctypes.data_as(C.POINTER(C.c_double))
    n = H.slslam_format_frame_text(len(ids), ip, dp, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert H.slslam_format_frame_text(len(ids), ip, dp, buf, n + 1) == n
    return buf.raw[:n]


def parsed(text=None, path=None, K=KITTI):
    H, fr, k = host(), Frame(), Intr(K["fx"], K["fy"], K["cx"], K["cy"])
    if path is not None:
        assert H.slslam_read_frame_file(path.encode(), C.byref(k), None, None, 0, C.byref(fr)) == 0
    else:
        assert H.slslam_parse_frame_text(text, len(text), C.byref(k), None, None, 0, C.byref(fr)) == 0
    ids = [fr.ids[i] for i in range(fr.num_lines)]
    obs = np.array([fr.observations[i] for i in range(8 * fr.num_lines)]).reshape(-1, 8)
    H.slslam_free_frame(C.byref(fr))
    return ids, obs


def test_written_frames_read_back_as_the_matchers_normalised_observations(tmp_path):
    """The text of the pixel observations (fx = fy = 1, cx = cy = 0), parsed under the KITTI intrinsics, is bit for bit what the stereo
    matcher gives for the same pairs under those intrinsics: both use insert_curr_obs's operation order."""
    for t, p in enumerate(chain_reference()):
        s = sequence()
        m = p["stereo"]
        ls = LSD.detect(s["images"][t])["segments"][p["left_rows"]].astype(np.float32)
        rs = LSD.detect(s["right_images"][t])["segments"][p["right_rows"]].astype(np.float32)
        rows = p["index"]
        under_k = np.array([SR.emit(ls[a], rs[m["match"][a]], SR.options(**KITTI))[0] for a in rows]).reshape(-1, 8)
        assert np.array_equal(p["observations"].astype(np.float32).astype(np.float64), p["observations"])   # pixels are float values
        order = np.argsort(p["ids"], kind="stable")                                            # the reader sorts by id
        text = frame_text(p["ids"], p["observations"])
        ids, obs = parsed(text)
        assert ids == p["ids"][order].tolist() and obs.tobytes() == under_k[order].tobytes()
        assert max(len(ln) for ln in text.split(b"\n")) < 255 and text.endswith(b"\n") and text.count(b"\n") == len(ids)
        path = str(tmp_path / ("%04d.txt" % t))
        ip, dp = p["ids"].astype(np.int32), np.ascontiguousarray(p["observations"])
        assert host().slslam_write_frame_file(path.encode(), len(ip), ip.ctypes.data_as(C.POINTER(C.c_int)),
                                              dp.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert open(path, "rb").read() == text and parsed(path=path)[0] == ids


def test_writer_format_ids_and_arguments(tmp_path):
    px = np.array([[100.25, 10.5, 120.125, 50.0, 80.0, 10.5, 90.0625, 50.0], [1, 2, 3, 4, 5, 6, 7, 8], [9, 9, 9, 9, 9, 9, 9, 9]], dtype=np.float64)
    px[1, 0] = float(np.float32(1.0) / np.float32(3.0))
    text = frame_text([7, 3, 7], px)
    assert text.split(b"\n")[0] == b"7 100.25 10.5 120.125 50 80 10.5 90.0625 50"
    assert text.split(b"\n")[1].split()[1] == b"%.17g" % px[1, 0] != b"0.333333343"            # nine digits would not read back as this double
    ids, obs = parsed(text, K=dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0))
    assert ids == [3, 7] and obs.tobytes() == px[[1, 0]].tobytes()                             # ascending; a duplicate id keeps its first line
    assert frame_text([], np.zeros((0, 8))) == b""
    wide = frame_text([-2147483648], np.full((1, 8), -float(np.float32(1.2345678e-38))))       # the longest a line gets
    assert len(wide) < 255 and parsed(wide, K=dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0))[1].tobytes() == np.full((1, 8), -float(np.float32(1.2345678e-38))).tobytes()
    H = host()
    one, o8 = np.array([1], np.int32), np.zeros(8)
    ip, dp = one.ctypes.data_as(C.POINTER(C.c_int)), o8.ctypes.data_as(C.POINTER(C.c_double))
    assert H.slslam_format_frame_text(1, None, dp, None, 0) == -1 and H.slslam_format_frame_text(1, ip, None, None, 0) == -1
    assert H.slslam_format_frame_text(-1, ip, dp, None, 0) == -1
    small = C.create_string_buffer(b"x" * 8, 8)
    assert H.slslam_format_frame_text(1, ip, dp, small, 4) == 18 and small.raw == b"1 0\0xxxx"  # truncated as snprintf truncates
    assert H.slslam_write_frame_file(None, 1, ip, dp) == 2 and H.slslam_write_frame_file(b"/nonexistent-dir/x.txt", 1, ip, dp) == 1
    assert H.slslam_write_frame_file(str(tmp_path / "e.txt").encode(), 0, None, None) == 0 and open(tmp_path / "e.txt", "rb").read() == b""
