// Several alignments of ONE source against ONE voxelized target in the same launches (ngicp_voxel_align_batch).
//
// ngicp_batch.h's scheme with the voxelized pass in the exact pass's place.  A LANE is one alignment: its own optimiser state, voxel
// numbers, n_v M matrices, partial rows and trace; the source, its covariances, the voxel map, the neighbourhood and every parameter are
// shared.
//   k_vgicp_pass_batch<K>   grid (ceil(n_src / kVoxBlock), live lanes), K = 1, 7, 27.  A block takes its lane from the launch's arguments
//                           (BatchLaunch::lane[blockIdx.y]), returns at its head when that lane's state says `done`, reads the lane's
//                           VoxelPassArgs record and the state's pose and flags (load_pose, as the single kernels), and runs the body the single kernel runs
//                           (vgicp_pass_body / vgicp_pass_n_body<K>, ngicp_voxel.h): the same per-point statements in the same slot
//                           order, the same [16][30] tile reduction, the same four-wave sum, the same [block][kNumSlots] row - in the
//                           lane's own buffers.  The rows k_lm_solve_batch then reads are bit for bit the single path's.
// The record and the state are read through the constant address space (scalar loads where the body wants a field, as the single kernel
// reads its arguments from the kernarg segment): neither changes while the launch runs - the solver that advances the state is the next
// launch on the stream.
// The test hooks of the single kernels (mode bit 2) and their first-pass stamp (t_first) have no counterpart here.
#pragma once
#include "ngicp_batch.h"
#include "ngicp_voxel.h"

namespace ngk {

template <int K>
struct VoxelBatchKernelTraits {
  typedef VoxelPassLdsN<K> Lds;
};
template <>
struct VoxelBatchKernelTraits<1> {
  typedef VoxelPassLds Lds;
};

template <int K>
__global__ void __launch_bounds__(kVoxBlock, K == 1 ? 1 : 2) k_vgicp_pass_batch(BatchLaunch bl) {
  static_assert(K == 1 || K == 7 || K == 27, "DIRECT1, DIRECT7 or DIRECT27");
  __shared__ typename VoxelBatchKernelTraits<K>::Lds sh;
  KernelBatchLaunch* kb = (KernelBatchLaunch*)__builtin_amdgcn_kernarg_segment_ptr();
  const int lane_id = kb->lane[blockIdx.y];
  KernelVoxelPassArgs* ka = (KernelVoxelPassArgs*)(unsigned long long)(reinterpret_cast<const VoxelPassArgs*>(kb->pass) + lane_id);
  KernelStatePtr st4 = (KernelStatePtr)(unsigned long long)ka->st;
  if (st4->hot.done) return;
  PassPose p;
  load_pose(st4, p);
  if constexpr (K == 1)
    vgicp_pass_body(*ka, p, sh);
  else
    vgicp_pass_n_body<K>(*ka, p, sh);
}

}  // namespace ngk
