"""Shared by tests/test_probability_grid_host.py, tests/test_gpu_probability_grid.py, tools/fuzz_probability_grid.py and
tools/probability_grid_bench.py: numpy restatements (float32, the reference's operation order) of what the CPU oracle
does not hold -- the known-cells box, the cropped image, its rotation, the ROS map texts -- and the comparison of a
device grid with an oracle grid."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
K_MIN = f32(0.1)                 # kMinProbability
K_MAX = f32(1.0) - K_MIN         # kMaxProbability
CC_MIN = f32(1.0) - K_MAX        # kMinCorrespondenceCost
CC_MAX = f32(1.0) - K_MIN        # kMaxCorrespondenceCost


def value_to_correspondence_cost():
    """probability_values.cc:27-36 for the values 0 .. 32767."""
    v = np.arange(32768, dtype=np.int64).astype(f32)
    scale = f32((CC_MAX - CC_MIN) / f32(32766.0))
    t = (v * scale + f32(CC_MIN - scale)).astype(f32)
    t[0] = CC_MAX
    return t


def color_table():
    """io/probability_grid_points_processor.cc:49-54 and :140-144: 128 for an unknown cell, else
    RoundToInt(255 * ((1 - p) - kMin) / (kMax - kMin)) with p = GetProbability = 1 - correspondence cost."""
    p_from_grid = (f32(1.0) - value_to_correspondence_cost()).astype(f32)
    q = (f32(1.0) - p_from_grid).astype(f32)
    x = (f32(255.0) * ((q - K_MIN).astype(f32) / f32(K_MAX - K_MIN)).astype(f32)).astype(f32)
    r = np.where(x >= 0, np.floor(x.astype(np.float64) + 0.5), np.ceil(x.astype(np.float64) - 0.5))  # lround: half away from zero
    out = r.astype(np.int64).astype(np.uint8)
    out[0] = 128
    return out


def probabilities():
    """GetProbability of the values 0 .. 32767 (probability_grid.cc:69-73)."""
    return (f32(1.0) - value_to_correspondence_cost()).astype(f32)


def known_box(cells):
    """Bounding box of the non-zero cells (every applied table value is >= 1 after FinishUpdate) ->
    (offset (x, y), size (w, h)) as ComputeCroppedLimits returns them (grid_2d.cc:101-111)."""
    ys, xs = np.nonzero(cells)
    if len(xs) == 0:
        return (0, 0), (1, 1)
    return (int(xs.min()), int(ys.min())), (int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def draw(cells, rotate_cw=False):
    """DrawProbabilityGrid (:127-148) -> (uint8 image [h, w], offset); Image::Rotate90DegreesClockwise (io/image.cc:67-76):
    the new rows are the old columns, each read from the bottom up."""
    (x0, y0), (w, h) = known_box(cells)
    img = color_table()[cells[y0:y0 + h, x0:x0 + w]]
    if rotate_cw:
        img = np.ascontiguousarray(img[::-1, :].T)
    return img, (x0, y0)


def to_string(v):
    return "%f" % v  # std::to_string(double)


def ros_map_files(cells, resolution, max_xy, pgm_filename):
    """(PGM bytes, YAML bytes) of ros_map_writing_points_processor.cc:60-80 with ros_map.cc:21-47."""
    img, (ox, oy) = draw(cells, rotate_cw=True)
    h, w = img.shape
    pgm = ("P5\n# Cartographer map; " + to_string(resolution) + " m/pixel\n%d %d\n255\n" % (w, h)).encode() + img.tobytes()
    origin = (max_xy[0] - (oy + w) * resolution, max_xy[1] - (ox + h) * resolution)
    yaml = ("image: " + pgm_filename + "\nresolution: " + to_string(resolution) + "\norigin: [" + to_string(origin[0]) + ", " +
            to_string(origin[1]) + ", 0.0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n").encode()
    return pgm, yaml


def new_oracle_grid(orc, resolution, limits=None):
    """io::CreateProbabilityGrid(resolution), or explicit (max_x, max_y, num_x, num_y)."""
    if limits is None:
        m = 0.5 * 100 * resolution
        return orc.ProbabilityGrid(resolution, (m, m), 100, 100)
    return orc.ProbabilityGrid(resolution, (limits[0], limits[1]), limits[2], limits[3])


def assert_equal(grid, ogrid):
    """Limits, every cell, the cropped offset / size and the error word of a device grid against the oracle's.
    -> the oracle's cells"""
    want = ogrid.cells()
    resolution, max_xy, num = grid.limits()
    assert resolution == ogrid.resolution and max_xy == tuple(ogrid.max_xy) and num == (ogrid.num_x_cells, ogrid.num_y_cells)
    got, off = grid.cells()
    assert off == (0, 0) and got.shape == want.shape and np.array_equal(got, want)
    offset, size = known_box(want)
    crop, crop_off = grid.cells(cropped=True)
    assert crop_off == offset and crop.shape == (size[1], size[0])
    assert np.array_equal(crop, want[offset[1]:offset[1] + size[1], offset[0]:offset[0] + size[0]])
    assert grid.stats()["error_word"] == 0
    return want
