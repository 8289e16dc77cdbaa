"""The record layouts of the relocalisation entries against the C header: sizeof / offsetof as gcc sees include/vieo_hot.h
must be what the numpy dtypes of vieo_slam_amd/relocalization.py say (no GPU: the header is plain C)."""
import os
import subprocess

from vieo_slam_amd import relocalization as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_records_match_the_header(tmp_path):
    prog = r"""
#include <stdio.h>
#include <stddef.h>
#include "vieo_hot.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("vieo_pnp_candidate %zu\n", sizeof(vieo_pnp_candidate));
  F(vieo_pnp_candidate, n); F(vieo_pnp_candidate, n_frame_keys); F(vieo_pnp_candidate, Xw); F(vieo_pnp_candidate, uv);
  F(vieo_pnp_candidate, sigma2); F(vieo_pnp_candidate, key_index); F(vieo_pnp_candidate, fx); F(vieo_pnp_candidate, fy);
  F(vieo_pnp_candidate, cx); F(vieo_pnp_candidate, cy);
  printf("vieo_pnp_params %zu\n", sizeof(vieo_pnp_params));
  F(vieo_pnp_params, probability); F(vieo_pnp_params, min_inliers); F(vieo_pnp_params, max_iterations);
  F(vieo_pnp_params, min_set); F(vieo_pnp_params, epsilon); F(vieo_pnp_params, th2); F(vieo_pnp_params, reserved);
  printf("vieo_pnp_info %zu\n", sizeof(vieo_pnp_info));
  F(vieo_pnp_info, n); F(vieo_pnp_info, n_frame_keys); F(vieo_pnp_info, min_inliers); F(vieo_pnp_info, max_its);
  F(vieo_pnp_info, n_rows); F(vieo_pnp_info, n_records); F(vieo_pnp_info, mask_words); F(vieo_pnp_info, iterations);
  F(vieo_pnp_info, best_inliers); F(vieo_pnp_info, best_row);
  printf("vieo_bow_keys %zu\n", sizeof(vieo_bow_keys));
  F(vieo_bow_keys, n_keys); F(vieo_bow_keys, n_nodes); F(vieo_bow_keys, keys); F(vieo_bow_keys, descriptors);
  F(vieo_bow_keys, mp_id); F(vieo_bow_keys, node_id); F(vieo_bow_keys, node_first); F(vieo_bow_keys, node_feat);
  printf("vieo_reloc_frame %zu\n", sizeof(vieo_reloc_frame));
  F(vieo_reloc_frame, n_keys); F(vieo_reloc_frame, n_levels); F(vieo_reloc_frame, keys); F(vieo_reloc_frame, uright);
  F(vieo_reloc_frame, descriptors); F(vieo_reloc_frame, level_sigma2); F(vieo_reloc_frame, inv_level_sigma2);
  F(vieo_reloc_frame, scale_factor); F(vieo_reloc_frame, log_scale_factor); F(vieo_reloc_frame, fx); F(vieo_reloc_frame, fy);
  F(vieo_reloc_frame, cx); F(vieo_reloc_frame, cy); F(vieo_reloc_frame, bf); F(vieo_reloc_frame, bounds);
  F(vieo_reloc_frame, n_nodes); F(vieo_reloc_frame, n_cams); F(vieo_reloc_frame, Rcb); F(vieo_reloc_frame, tcb);
  F(vieo_reloc_frame, node_id); F(vieo_reloc_frame, node_first); F(vieo_reloc_frame, node_feat);
  printf("vieo_reloc_candidate %zu\n", sizeof(vieo_reloc_candidate));
  F(vieo_reloc_candidate, kf); F(vieo_reloc_candidate, points);
  printf("vieo_reloc_visit %zu\n", sizeof(vieo_reloc_visit));
  F(vieo_reloc_visit, cand); F(vieo_reloc_visit, call); F(vieo_reloc_visit, row); F(vieo_reloc_visit, no_more);
  F(vieo_reloc_visit, found); F(vieo_reloc_visit, n_inliers); F(vieo_reloc_visit, n_good); F(vieo_reloc_visit, n_additional);
  F(vieo_reloc_visit, reserved);
  printf("vieo_reloc_result %zu\n", sizeof(vieo_reloc_result));
  F(vieo_reloc_result, found); F(vieo_reloc_result, cand); F(vieo_reloc_result, n_good); F(vieo_reloc_result, n_visits);
  F(vieo_reloc_result, nav); F(vieo_reloc_result, Tcw);
  return 0;
}
"""
    src = tmp_path / "sizes.c"
    src.write_text(prog)
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    got = {k: int(v) for k, v in got.items()}
    dtypes = {"vieo_pnp_candidate": rl.PNP_CANDIDATE_DTYPE, "vieo_pnp_params": rl.PNP_PARAMS_DTYPE,
              "vieo_pnp_info": rl.PNP_INFO_DTYPE, "vieo_bow_keys": rl.BOW_KEYS_DTYPE,
              "vieo_reloc_frame": rl.RELOC_FRAME_DTYPE, "vieo_reloc_candidate": rl.RELOC_CANDIDATE_DTYPE,
              "vieo_reloc_visit": rl.RELOC_VISIT_DTYPE, "vieo_reloc_result": rl.RELOC_RESULT_DTYPE}
    assert [got[k] for k in dtypes] == [56, 32, 40, 56, 224, 64, 48, 256]
    n_fields = 0
    for name, dt in dtypes.items():
        assert got[name] == dt.itemsize, name
        for f in dt.names:
            assert got["%s.%s" % (name, f)] == dt.fields[f][1], (name, f)
            n_fields += 1
    assert n_fields == len(got) - len(dtypes)
