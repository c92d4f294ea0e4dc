"""The timing switch of the four handles of the image front end (csrc/call_block.h: TimedHandle), each on the smallest input that
launches anything: off it measures nothing and changes nothing, on it measures the launches, and switched off again the handle keeps
the last figure.  The results of the three runs are the same bytes, and the handle allocates once."""
import numpy as np
import pytest

from slslam_amd import capi

pytestmark = pytest.mark.gpu

IMAGE = np.zeros((32, 32), dtype=np.uint8)
IMAGE[:, 16:] = 255                                                             # one drawn edge
SEGMENT = np.array([[16.0, 4.0, 16.0, 28.0]], dtype=np.float32)
DESCRIPTOR = np.array([[0.6, 0.0, 0.8, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
LEFT = (np.array([[20.0, 5.0, 20.0, 25.0]], dtype=np.float32), DESCRIPTOR)
RIGHT = (np.array([[15.0, 5.0, 15.0, 25.0]], dtype=np.float32), DESCRIPTOR)


def frozen(x):
    """A result as something == compares byte for byte."""
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def track_twice(tracker):
    tracker.reset(0)
    return [tracker.run([LEFT]), tracker.run([LEFT])]


CASES = {
    "detector": (lambda: capi.LineDetector(max_frames=1, max_pixels=32 * 32), lambda h: h.run([IMAGE])),
    "descriptor": (lambda: capi.LineDescriptor(max_frames=1, max_pixels=32 * 32, max_segments=1), lambda h: h.run([(IMAGE, SEGMENT)])),
    "stereo": (lambda: capi.StereoMatcher(8, max_frames=1, max_segments=1), lambda h: h.run([(LEFT, RIGHT)])),
    "tracker": (lambda: capi.LineTracker(8, max_frames=1, max_segments=1), track_twice),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_switch(name):
    make, run = CASES[name]
    h = make()
    first = frozen(run(h))
    assert h.kernel_ms() == 0.0 and h.stats()["allocations"] == 1
    h.set_timing(True)
    second = frozen(run(h))
    ms = h.kernel_ms()
    assert ms > 0.0 and h.stats()["allocations"] == 1
    h.set_timing(False)
    third = frozen(run(h))
    assert h.kernel_ms() == ms and h.stats()["allocations"] == 1
    assert first == second == third
    h.close()
