"""bench.py --dump-outputs DIR: what the timed path computed in its last timed step, one .npy per array, so that two
builds of the project can be compared output for output (the scene and the scans are seeded: the same arguments give
the same inputs).

  rtcsm_score      (1,) float32  RealTimeCorrelativeScanMatcher3D::Match's score
  rtcsm_pose       (7,) float64  its pose [t, q(w,x,y,z)]
  ceres_pose       (7,) float64  CeresScanMatcher3D::Match's pose: what the step hands on
  ceres_summary    (8,) float64  the summary in CsmSummary's field order (CERES_SUMMARY_FIELDS)
  grid_<name>_origins  (m, 3) float32  voxel index of each leaf's (0,0,0) corner, sorted (x, y, z)
  grid_<name>_values   (m, 512) float32  the leaf's uint16 cells, z-major (include/dliom.h "block")

The grids are read after the last timed step's insertion.  They share GRID_BUDGET_BYTES; a grid whose leaves do not
fit is written as a fixed, seeded sample of them (grid_<name>_num_leaves holds the count before sampling)."""
import os

import numpy as np

CERES_SUMMARY_FIELDS = ("initial_cost", "final_cost", "num_successful_steps", "num_unsuccessful_steps", "num_iterations",
                        "num_residual_evaluations", "num_jacobian_evaluations", "termination_type")
GRID_BUDGET_BYTES = 60 << 20  # of the 64 MB the dump may take
SAMPLE_SEED = 20261015


def grid_arrays(name, grid, budget_bytes):
    origins, values = grid.download_blocks()
    order = np.lexsort((origins[:, 2], origins[:, 1], origins[:, 0]))
    n = len(order)
    keep = max(1, budget_bytes // (4 * (3 + 512)))
    if n > keep:
        order = order[np.sort(np.random.RandomState(SAMPLE_SEED).choice(n, keep, replace=False))]
    return {"grid_%s_origins" % name: origins[order].astype(np.float32),
            "grid_%s_values" % name: values[order].astype(np.float32),
            "grid_%s_num_leaves" % name: np.array([n], dtype=np.float64)}


def dump(directory, last, grids):
    """last: the last timed step's {'rtcsm_score', 'rtcsm_pose', 'ceres_pose', 'ceres_summary'}; grids: [(name, grid)].
    Returns the result line's `dump_outputs` entry."""
    arrays = {"rtcsm_score": np.array([last["rtcsm_score"]], dtype=np.float32),
              "rtcsm_pose": np.asarray(last["rtcsm_pose"], dtype=np.float64),
              "ceres_pose": np.asarray(last["ceres_pose"], dtype=np.float64),
              "ceres_summary": np.array([last["ceres_summary"][f] for f in CERES_SUMMARY_FIELDS], dtype=np.float64)}
    for name, grid in grids:
        arrays.update(grid_arrays(name, grid, GRID_BUDGET_BYTES // len(grids)))
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)
    return {"dir": directory, "arrays": sorted(arrays), "bytes": int(sum(a.nbytes for a in arrays.values()))}
