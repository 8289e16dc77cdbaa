// pnp_usun.h -- usun of PnPsolver::add_correspondence with Frame::usedistort_ (reference src/PnPsolver.cc:349-358): the
// key's pixel un-projected through its own camera, moved into the reference camera with GetTrc(), K of camera 0
// applied and divided.  One lane function for k_pnp_usun of pnp.hip; like pnp_device.h the file also compiles as plain
// C++ (cam_unproject.h does), which is how it is exercised on a host.
#pragma once
#include "cam_unproject.h"
#include "pnp_device.h"

namespace vieo {

// K0 = (fx, fy, cx, cy) of mpCameras[0]->toK(), float parameters widened.  (The reference multiplies the 3 x 3 K: the
// zero entries add nothing to a finite point.)
PNP_DEV void pnp_usun(const PnpRigDev& G, int cam, float u, float v, float fx, float fy, float cx, float cy, double* usun) {
  double Pc[3], Pr[3];
  cam_unproject(G.cams[cam], u, v, Pc);
  pnp_rig_transform(G.Trc[cam], Pc, Pr);
  const double x = (double)fx * Pr[0] + (double)cx * Pr[2], y = (double)fy * Pr[1] + (double)cy * Pr[2];
  const double invz = 1. / Pr[2];
  usun[0] = x * invz, usun[1] = y * invz;
}

}  // namespace vieo
