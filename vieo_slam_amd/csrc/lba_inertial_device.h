// lba_inertial_device.h -- the pair edges of the bundle-adjustment engine (lba.hip): EdgeNavStatePRV + EdgeNavStateBias of
// a visual-inertial window's key-frame pair and EdgeEncNavStatePR of an encoder pair (reference src/Optimizer.cc:219-347;
// the edges' algebra is imu_device.h's), one wavefront per pair.
//   lba_generic_dev  the body for one wavefront; static LDS 9640 B (the edge's record, J, (rho' Info) J, errors)
//   k_lba_generic    grid (pairs of the largest window, windows) x 64 threads; mode 0 under LBA_BUILD, mode 1 under LBA_TRIAL
// Reads   imu[e], kf[imu[e].i], kf[imu[e].j], gw, qRbe, pbe, n_imu.
// Writes  mode 0: Ae[e] (30 x 30 block + gradient 30, local order [kf_i: PR V Bias | kf_j: PR V Bias]) and gchi0[e];
//         mode 1: gchi[e].
// Launched by launch_round (lba.hip): k_lba_generic(0) after the two-launch build, k_lba_generic(1) in the four-launch
// tail of a trial.  Calls of a few windows run the same body inside k_lba_build<.., 2> (lba_linearize_device.h: the
// workgroups behind the chunk workgroups, mode 0) and k_lba_tail (lba_state_device.h: behind the point workgroups,
// mode 1) -- this header comes ahead of both.
#pragma once
#include "imu_device.h"
#include "lba_device.h"

namespace vieo {

// ---- inertial edges of a visual-inertial window: one wavefront per key-frame pair.
// mode 0: linearise at the current state (30x30 block J^T (rho' Omega) J and gradient, both edges of the
// pair) and robust chi2 -> gchi0; mode 1: robust chi2 after a trial -> gchi.
// (the body, for one wavefront: k_lba_generic's workgroups and the pair workgroups of k_lba_tail)
__device__ __forceinline__ void lba_generic_dev(const LbaDev& D, int e, int lane, int mode) {
  __shared__ double sJ[9 * 30], sT[9 * 30], sErr[9 + 6], sWe[9], sRho[3];
  __shared__ double sJE[6 * 30], sTE[6 * 30], sWeE[6];  // encoder edge: J in the local order, (rho' Info) J, Info e
  // the edge's record staged in LDS by the whole wavefront: lane 0's chains below read it field by field, and every
  // dependent batch of those reads was a trip to L2
  static_assert(sizeof(LbaImu) % 8 == 0, "staged in 8-byte words");
  __shared__ __align__(16) double sE_store[sizeof(LbaImu) / 8];
  {
    const double* src = reinterpret_cast<const double*>(&D.imu[e]);
    for (int i = lane; i < (int)(sizeof(LbaImu) / 8); i += 64) sE_store[i] = src[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const LbaImu& E = *reinterpret_cast<const LbaImu*>(sE_store);
  const double dI = (double)(float)sqrt(16.919), dB = (double)(float)sqrt(12.592);  // Optimizer.cc:219-222
  if (lane == 0) {
    NSd si, sj;
    const LbaKf &ki = D.kf[E.i], &kj = D.kf[E.j];
    for (int k = 0; k < 3; k++) {
      si.p[k] = ki.p[k], si.v[k] = ki.v[k], si.bg[k] = ki.bg[k], si.ba[k] = ki.ba[k];
      si.dbg[k] = ki.dbg[k], si.dba[k] = ki.dba[k];
      sj.p[k] = kj.p[k], sj.v[k] = kj.v[k], sj.bg[k] = kj.bg[k], sj.ba[k] = kj.ba[k];
      sj.dbg[k] = kj.dbg[k], sj.dba[k] = kj.dba[k];
    }
    si.qw = ki.qw, si.qx = ki.qx, si.qy = ki.qy, si.qz = ki.qz;
    sj.qw = kj.qw, sj.qx = kj.qx, sj.qy = kj.qy, sj.qz = kj.qz;
    double chi = 0, rI = 1.0, rB = 1.0;
    if (E.has_imu) {
      imu_error(E.M, D.gw, si, sj, sErr, 3);
      double c2 = 0;
      for (int a = 0; a < 9; a++) {
        double t = 0;
        for (int b = 0; b < 9; b++) t += E.InfoI[a * 9 + b] * sErr[b];
        sWe[a] = t;
        c2 += sErr[a] * t;
      }
      double r0 = c2;
      if (E.robust) huber(c2, dI, dI * dI, &r0, &rI);
      chi += r0;
    }
    for (int k = 0; k < 3; k++) {
      sErr[9 + k] = (sj.bg[k] + sj.dbg[k]) - (si.bg[k] + si.dbg[k]);
      sErr[12 + k] = (sj.ba[k] + sj.dba[k]) - (si.ba[k] + si.dba[k]);
    }
    {
      double c2 = 0;
      for (int k = 0; k < 3; k++) c2 += sErr[9 + k] * (E.infoBg * sErr[9 + k]);
      for (int k = 3; k < 6; k++) c2 += sErr[9 + k] * (E.infoBa * sErr[9 + k]);
      double r0 = c2;
      if (E.robust) huber(c2, dB, dB * dB, &r0, &rB);
      chi += r0;
    }
    double rE = 1.0;
    if (E.has_enc) {
      double errE[6], JEi[36], JEj[36];
      enc_edge_eval(si, sj, E.measE, D.qRbe, D.pbe, errE, mode == 0 ? JEi : nullptr, mode == 0 ? JEj : nullptr);
      double c2 = 0;
      for (int a = 0; a < 6; a++) {
        double t = 0;
        for (int b = 0; b < 6; b++) t += E.InfoE[a * 6 + b] * errE[b];
        sWeE[a] = t;
        c2 += errE[a] * t;
      }
      double r0 = c2;
      if (E.enc_robust) huber(c2, dB, dB * dB, &r0, &rE);  // sqrt(12.592), Optimizer.cc:343
      chi += r0;
      if (mode == 0)
        for (int a = 0; a < 6; a++) {
          for (int c = 0; c < 30; c++) sJE[a * 30 + c] = 0;
          for (int c = 0; c < 6; c++) sJE[a * 30 + c] = JEi[a * 6 + c], sJE[a * 30 + 15 + c] = JEj[a * 6 + c];
        }
    }
    (mode ? D.gchi : D.gchi0)[e] = chi;
    sRho[0] = rI, sRho[1] = rB, sRho[2] = rE;
    if (mode == 0 && E.has_imu) {
      // J (9 x 24, [PRV_j | PRV_i | Bias_i]) -> local order [i: PR V Bias | j: PR V Bias]
      double* J24 = sT;  // (LDS, free until the products below: as a local array it lived in scratch, 1.7 KB per lane)
      imu_linearize(E.M, D.gw, si, sj, sErr, J24, 3, 6);
      for (int a = 0; a < 9; a++) {
        for (int c = 0; c < 30; c++) sJ[a * 30 + c] = 0;
        for (int c = 0; c < 9; c++) sJ[a * 30 + 15 + c] = J24[a * 24 + c];       // state j: PR, V
        for (int c = 0; c < 9; c++) sJ[a * 30 + c] = J24[a * 24 + 9 + c];        // state i: PR, V
        for (int c = 0; c < 6; c++) sJ[a * 30 + 9 + c] = J24[a * 24 + 18 + c];   // Bias_i
      }
    }
  }
  if (mode) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double* A = D.Ae + 930 * (size_t)e;
  const double rI = sRho[0], rB = sRho[1], rE = sRho[2];
  if (E.has_enc) {
    for (int t = lane; t < 180; t += 64) {
      const int a = t / 30, c = t - a * 30;
      double u = 0;
      for (int q = 0; q < 6; q++) u += (rE * E.InfoE[a * 6 + q]) * sJE[q * 30 + c];
      sTE[t] = u;
    }
  }
  if (E.has_imu) {
    for (int t = lane; t < 270; t += 64) {  // T = (rho' Info) J
      const int a = t / 30, c = t - a * 30;
      double u = 0;
      for (int q = 0; q < 9; q++) u += (rI * E.InfoI[a * 9 + q]) * sJ[q * 30 + c];
      sT[t] = u;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < 900; t += 64) {
    const int c1 = t / 30, c2 = t - c1 * 30;
    double u = 0;
    if (E.has_imu)
      for (int a = 0; a < 9; a++) u += sJ[a * 30 + c1] * sT[a * 30 + c2];
    if (E.has_enc)
      for (int a = 0; a < 6; a++) u += sJE[a * 30 + c1] * sTE[a * 30 + c2];
    // bias edge: J_i = -I on rows/cols 9..14, J_j = +I on 24..29
    const int b1 = c1 >= 24 ? c1 - 24 : (c1 >= 9 && c1 < 15 ? c1 - 9 : -1);
    const int b2 = c2 >= 24 ? c2 - 24 : (c2 >= 9 && c2 < 15 ? c2 - 9 : -1);
    if (b1 >= 0 && b1 == b2) {
      const double wgt = (b1 < 3 ? E.infoBg : E.infoBa) * rB;
      u += ((c1 >= 24) == (c2 >= 24)) ? wgt : -wgt;
    }
    A[t] = u;
  }
  if (lane < 30) {
    double u = 0;
    if (E.has_imu)
      for (int a = 0; a < 9; a++) u += sJ[a * 30 + lane] * (-sWe[a] * rI);
    if (E.has_enc)
      for (int a = 0; a < 6; a++) u += sJE[a * 30 + lane] * (-sWeE[a] * rE);
    const int b1 = lane >= 24 ? lane - 24 : (lane >= 9 && lane < 15 ? lane - 9 : -1);
    if (b1 >= 0) {
      const double we = (b1 < 3 ? E.infoBg : E.infoBa) * sErr[9 + b1] * rB;
      u += lane >= 24 ? -we : we;
    }
    A[900 + lane] = u;
  }
}
__global__ void __launch_bounds__(64)
k_lba_generic(const LbaDev* __restrict__ devs, const WinCtl* __restrict__ ctl, int mode) {
  const int w = blockIdx.y, fl = ctl[w].flags;
  if (!(fl & (mode ? LBA_TRIAL : LBA_BUILD))) return;
  const LbaDev& D = devs[w];
  if ((int)blockIdx.x >= D.n_imu) return;
  lba_generic_dev(D, blockIdx.x, threadIdx.x, mode);
}

}  // namespace vieo
