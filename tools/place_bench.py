"""Time of the place recogniser's insert and run at the reference's tree shape, beside the numpy reference on one host thread.

    python tools/place_bench.py [--docs 2000] [--descriptors 300] [--frames 1 64] [--repeats 15] [--out profiles/place_bench.txt]

Tree (40, 3, 72) of random unit centres (synth.make_voctree); descriptors drawn from a pool of 5000 unit vectors with Gaussian noise, so
that documents share words; recent 40, 100 average words, top_k 10.  The database is filled until `docs` documents are visible.  Warm
(three untimed calls first), median and spread of `repeats` calls, two figures each: HIP events on the null stream around the call - the
call is synchronous on the database's own stream, so this is upload + launches + download as the device clock sees them - and the wall
time of the call.  The raw entry points on prepared arrays, so that the binding's conversions are not in the time.  "documents only" is the
same run against a database in which nothing is visible yet (k_place_document and the default-filling k_place_finish): the difference to
the full run is k_place_score + k_place_finish.  The numpy reference (tests/place_reference.py) is given the device's documents and
timed on the same frames (at most --numpy-frames of them, scaled).  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=2000)
    ap.add_argument("--descriptors", type=int, default=300)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--numpy-frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from slslam_amd import capi, synth
    import place_reference as R
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    K, L, D, recent, navg, top_k = 40, 3, 72, 40, 100, 10
    n, maxF = a.descriptors, max(a.frames)
    rng = np.random.default_rng(77)
    pool = rng.standard_normal((5000, D))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)

    def frame():
        d = pool[rng.integers(0, len(pool), n)] + 0.02 * rng.standard_normal((n, D))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    nodes = synth.make_voctree(1, K, L, D)
    tree = capi.VocTree(K, L, D, nodes)
    lines = ["place_bench: tree (%d, %d, %d) = %.1f MB, %d visible documents of %d descriptors, recent %d, %d average words, top_k %d"
             % (K, L, D, nodes.nbytes / 1e6, a.docs, n, recent, navg, top_k)]

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); call(); e1.record()
            e1.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(e0.elapsed_time(e1))
        return ev, wall

    def row(name, ms):
        return "%s: median %.3f ms (min %.3f, max %.3f, %d calls)" % (name, statistics.median(ms), min(ms), max(ms), len(ms))

    # fill: docs + recent + 1 inserts make `docs` documents visible; the last repeats + 3 inserts are the timed ones
    total = a.docs + recent + 1
    db = capi.PlaceDB(tree, max_docs=total + a.repeats + 8, max_words=512, max_frames=maxF, recent=recent, num_avg_words=navg)
    ref = R.Database(R.Tree(K, L, D, nodes), recent, navg)
    t0 = time.perf_counter()
    for _ in range(total - a.repeats - 3):
        ref.docs.append(R.document(db.insert(frame())["words"]))
    fill_s = time.perf_counter() - t0
    st, words = C.c_int(0), np.zeros(n, dtype=np.int32)

    def insert():
        fr = frame()
        pf, keep = capi._place_frame(tree, fr)
        rc = capi.lib().slslam_place_db_insert(db._h, C.byref(pf), C.byref(st), capi._ip(words))
        assert rc == 0 and st.value == 0, (rc, st.value)
        ref.docs.append(R.document(words.copy()))

    ev, wall = timed(insert)
    assert db.size()["visible"] == a.docs, db.size()
    lines.append("fill: %d inserts through the binding in %.2f s" % (total - a.repeats - 3, fill_s))
    lines.append(row("insert at %d visible documents (quantise, document, df / virtual document upkeep on the host), HIP events" % a.docs, ev))
    lines.append(row("insert, wall", wall))
    for d in range(a.docs):                                     # the reference's state from the device's documents
        ref.df[ref.docs[d][0]] += 1
    ref.visible = a.docs
    ref._rebuild_virtual()
    assert np.array_equal(ref.virtual, db.virtual_words())

    empty = capi.PlaceDB(tree, max_docs=8, max_words=512, max_frames=maxF, recent=recent, num_avg_words=navg)
    empty.insert(frame())
    for F in a.frames:
        frames = [frame() for _ in range(F)]
        pfs, outs, keep = (capi.PlaceFrame * F)(), (capi.PlaceResult * F)(), []
        S = a.docs + 1
        for i, fr in enumerate(frames):
            pfs[i], k = capi._place_frame(tree, fr)
            b = [np.zeros(n, np.int32), np.zeros(S, np.float32), np.zeros(S, np.uint8), np.zeros(S, np.float32), np.zeros(top_k, np.int32),
                 np.zeros(top_k, np.float32)]
            outs[i] = capi.PlaceResult(-1, 0, 0, capi._ip(b[0]), capi._fp(b[1]), b[2].ctypes.data_as(C.POINTER(C.c_ubyte)), capi._fp(b[3]),
                                       capi._ip(b[4]), capi._fp(b[5]))
            keep += [k, b]

        def run(h=db._h):
            rc = capi.lib().slslam_place_db_run(h, F, pfs, top_k, outs)
            assert rc == 0, rc

        ev, wall = timed(run)
        lines.append(row("run, %d frame(s) per call, HIP events" % F, ev))
        lines.append(row("run, %d frame(s) per call, wall" % F, wall))
        full = statistics.median(ev)
        ev0, _ = timed(lambda: run(empty._h))
        lines.append(row("  documents only (nothing visible), %d frame(s), HIP events" % F, ev0))
        lines.append("  -> k_place_score + k_place_finish + the larger download: %.3f ms of %.3f ms" % (full - statistics.median(ev0), full))
        run()
        m = min(F, a.numpy_frames)
        t0 = time.perf_counter()
        refs = [ref.query(frames[i], top_k=top_k) for i in range(m)]
        t_np = time.perf_counter() - t0
        same = all(np.array_equal(keep[2 * i + 1][1].view(np.uint32), refs[i]["score"].view(np.uint32)) and
                   np.array_equal(keep[2 * i + 1][0], refs[i]["words"]) for i in range(m))
        lines.append("  numpy reference, one host thread: %.1f ms per frame (%d timed) = %.1f ms for the call; device words and score bits equal "
                     "the reference's: %s" % (1e3 * t_np / m, m, 1e3 * t_np / m * F, same))
    lines.append("database buffers: %s" % db.stats())
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
