"""A numpy mirror of cavmd_trajectory (include/cavmd.h): the layout of a frame, the rule of one call and the bytes a recording
call leaves in its slot.  Written from the header's text, not from the library: tests/test_trajectory_abi.py holds it against
hand-worked cases, tests/test_gpu_trajectory.py holds the kernel against it bit for bit."""
import numpy as np

F64, F32 = 0, 1
HEADER_BYTES = 64
FORCED, HAS_VELOCITIES = 1, 2
HEADER_DTYPE = np.dtype([("call", "<u8"), ("row", "<u8"), ("time", "<f8"), ("N", "<u4"), ("flags", "<u4"), ("box", "<f8", (3,)),
                         ("reserved", "<u8")])
assert HEADER_DTYPE.itemsize == HEADER_BYTES


def pad16(x: int) -> int:
    return (x + 15) // 16 * 16


def layout(max_N: int, fmt: int) -> dict:
    e = {F64: 8, F32: 4}[fmt]
    position = HEADER_BYTES
    velocity = position + pad16(3 * max_N * e)
    image = velocity + pad16(3 * max_N * e)
    return dict(frame_bytes=image + pad16(12 * max_N), position_offset=position, velocity_offset=velocity, image_offset=image,
                max_N=max_N, format=fmt, element_bytes=e, reserved=0)


class Item:
    """the five counter words of one item"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.rows = self.calls = self.phase = self.slot = 0
        self.last_time = 0.0

    def call(self, capacity: int, period: int, time_interval: float, time, forced: bool):
        """One call.  `time` is what *d_time holds (None: d_time is NULL).  Returns None where no frame is written, else the
        header's dict(call, row, time, forced) and the slot the frame goes to."""
        self.calls += 1
        if time_interval == 0.0:
            self.phase += 1
            due = self.phase >= period
        else:
            with np.errstate(invalid="ignore"):
                due = self.rows == 0 or bool(np.float64(time) - np.float64(self.last_time) >= np.float64(time_interval))
        if not (due or forced):
            return None
        slot = self.rows % capacity
        assert slot == self.slot
        head = dict(call=self.calls, row=self.rows, time=0.0 if time is None else float(time), forced=bool(forced), slot=slot)
        self.last_time = head["time"]
        self.phase = 0
        self.rows += 1
        self.slot = self.rows % capacity
        return head


def convert(x: np.ndarray, fmt: int) -> np.ndarray:
    """the stated conversion of float64 components: exact copies, or (float)x -- IEEE round to nearest even, subnormal
    results kept, beyond the float range +-inf, NaN stays NaN"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if fmt == F64:
        return x
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return x.astype(np.float32)


def frame_bytes(lay: dict, old: np.ndarray, head: dict, box, pos, vel, image) -> np.ndarray:
    """The slot after a recording call: `old` (frame_bytes uint8, what the slot held) with the header, the 3 N components of
    each section and the zero bytes up to the section's next 16-byte boundary written; everything else as it was.
    pos, vel: (N, 4) float64 (vel None: the section is +0); image: (N, 3) int32."""
    out = np.array(old, dtype=np.uint8, copy=True)
    assert out.shape == (lay["frame_bytes"],)
    N = 0 if pos is None else int(np.shape(pos)[0])
    assert N <= lay["max_N"]
    h = np.zeros(1, dtype=HEADER_DTYPE)
    h["call"], h["row"], h["time"], h["N"] = head["call"], head["row"], head["time"], N
    h["flags"] = (FORCED if head["forced"] else 0) | (HAS_VELOCITIES if vel is not None else 0)
    h["box"] = box
    out[:HEADER_BYTES] = h.view(np.uint8)
    if N == 0:
        return out
    e = lay["element_bytes"]
    zeros = np.zeros((N, 3))
    for offset, section in ((lay["position_offset"], convert(np.asarray(pos)[:, :3], lay["format"])),
                            (lay["velocity_offset"], convert(zeros if vel is None else np.asarray(vel)[:, :3], lay["format"])),
                            (lay["image_offset"], np.ascontiguousarray(np.asarray(image)[:, :3], dtype=np.int32))):
        raw = section.reshape(-1).view(np.uint8)
        assert raw.size == 3 * N * (e if offset != lay["image_offset"] else 4)
        out[offset:offset + raw.size] = raw
        out[offset + raw.size:offset + pad16(raw.size)] = 0
    return out
