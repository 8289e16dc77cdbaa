// sbp_grid.h -- the window grid of the projection searches: Frame::mGrid (FrameBase.h:224-225, 64 x 48 cells per camera)
// as a CSR with the keys' records in cell order.  Shared by the tracker-side searches (proj_search.hip, which defines
// k_sbp_grid and sbp_build_grids) and the map-side ones (map_search.hip, which only calls sbp_build_grids).  The
// thresholds and the descriptor distance of both come with orb_match.h.
#pragma once
#include "common.h"
#include "orb_match.h"

namespace vieo {

static const int kGridRows = 48, kGridCols = 64;  // FrameBase.h:224-225
static const int kGridCells = kGridCols * kGridRows;
static const int kMaxKeys = 8192;                 // 13-bit key index packing (4 cameras x 1500 features fit); a camera's grid holds no more
static const int kMaxCams = 4;

// The grid of a set of frames (device memory).  Frame f holds key_cap key positions, its cameras' keys in consecutive
// ranges of them; the keys of (f, cam) start at position k0.
struct SbpGrid {
  int* cell_start;   // [frame][cam][kGridCells + 1] first record of every cell (column-major: ix * kGridRows + iy), camera-local
  float4* cell_rec;  // [frame][key_cap] at f * key_cap + k0: the camera's keys in cell order, ascending by position inside a
                     // cell: x, y, uright, position | octave << 16
  float* cell_ang;   // [frame][key_cap] their angles
  int key_cap, n_cams;
};

// What sbp_build_grids reads (device memory) and the one thing it writes besides the grid.
struct SbpGridKeys {
  const vieo_keypoint* keys;  // [frame][key_cap]: x, y, octave and angle of every key inside a camera's range
  const float* uright;        // [frame][key_cap]: copied into the records' z
  const int* cam_first;       // [frame][n_cams + 1] ascending: camera c holds the positions [cam_first[c], cam_first[c + 1]),
                              // at most kMaxKeys of them, every position below 65536; positions >= key_cap are dropped
  float bounds[kMaxCams][4];  // per camera min x, max x, min y, max y of the image (gridinfo_.minmax_xy_)
  int* cursor;                // [frame]: cursor[f] is set to ZERO (the tracker's candidate pool of the frame is emptied)
};

// Builds G for n_frames frames on `st`: one launch of k_sbp_grid<1024>, a workgroup per (frame, camera).  The record
// indices are POSITIONS in the frame's key list (camera-local index + k0), not indices of any order the caller permuted
// the keys from.  Keys outside the image bounds are in no cell.  Nothing else of the tracker's search arguments is read.
int sbp_build_grids(const SbpGridKeys& in, int n_frames, const SbpGrid& G, hipStream_t st);

}  // namespace vieo
