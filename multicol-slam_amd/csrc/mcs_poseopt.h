// mcs_poseopt.h — what the pieces of mcs_pose_optimization share: the call's arguments, its argument checks (mcs_poseopt_guard.hip: host logic only, no HIP
// call; tests/test_poseopt_cpu.py runs it alone) and the kernel's launcher (mcs_poseopt.hip).
#pragma once
#include "mcs_host.h"

namespace mcs {

struct PoseCall {
	int nproblems; const mcs_pose_frame* frames; const mcs_point_table* pts; const double* McMin; const mcs_ocam* cams; int nrCams;
	const double* invSigma2; int nlevels; const double* huber; mcs_mem_kind kind;
	double* poseMin; double* MtMc; double* MtMcInv; uint8_t* const* outlier; int32_t* nInliers; double* share; mcs_pose_diag* diag;
};
// MCS_OK, or the refusal's code with its text left for mcs_last_error(); `c` is only compared with null.  asyncSearch: deferred searches are on.
// nproblems == 0 passes (the entry point returns before it reads anything else).
int guard_pose(const mcs_ctx* c, const PoseCall& q, bool asyncSearch);
// the scan of a host-kind call's contents: what the kernel indexes with (device kind: such a feature contributes no edge)
int guard_pose_content(const PoseCall& q);

// The kernel takes the per-problem pointers BY VALUE, kPoseBatch problems per launch: a device-kind call uploads no table and so never waits for the stream.
constexpr int kPoseBatch = 64;
constexpr int kPoseThreads = 512;
struct PoseChunk {
	const mcs_keypoint* keys[kPoseBatch]; const int* cam[kPoseBatch]; const int* points[kPoseBatch]; uint8_t* outlier[kPoseBatch]; int n[kPoseBatch];
};
struct PoseArgs {
	const double* pos; int npoints; const double* McMin; const mcs_ocam* cams; int nrCams; const double* invSigma2; int nlevels; const double* huber;
	double* poseMin; double* MtMc; double* MtMcInv; int* nInliers; double* share; mcs_pose_diag* diag;   // indexed by the problem's place in the whole batch
};
void launch_poseopt(const PoseArgs& a, const PoseChunk& ch, int first, int count, hipStream_t s);   // problems [first, first + count), count <= kPoseBatch

}  // namespace mcs
