// ntm_generic.h -- launchers of the runtime-class-count NTM kernels (ntm_generic.hip), called by the C ABI entry
// points in ntm.hip whenever c != 17.
#pragma once
#include <hip/hip_runtime.h>

namespace geot {

constexpr int GEN_MAXC = 32;   // a half-wave per matrix row

// What gen_sig_t_mean launches for a shape (ntm_generic.hip: gen_sig_plan, read by the launchers and by geot_ntm_generic_plan)
enum { GEN_FORM_REFUSED = -1, GEN_FORM_NONE = 0, GEN_FORM_WAVE = 1, GEN_FORM_ROWS = 2, GEN_FORM_MFMA = 3 };
struct GenSigPlan {
    int form;            // GEN_FORM_*
    int cp;              // rows: CP (registers per point); mfma: CPAD (rows per head of a row tile); wave: 0
    int tails;           // mfma: C is no multiple of 4
    int ksplit;          // mfma: ranges of row tiles (1 for the other forms)
    long long blocks;    // workgroups
    size_t lds;          // dynamic LDS bytes per workgroup
};
GenSigPlan gen_sig_plan(int b, int n, int c, int cus);   // cus <= 0: the current device's
int gen_blocks(long long total_pts);                      // workgroups of gen_correct_fwd / _bwd

hipError_t gen_sig_t_mean(bool backward, int b, int n, int c, const float *p, const float *W, const float *cm,
                          const float *grad_out, float *out, hipStream_t s);
hipError_t gen_correct_fwd(int b, int n, int c, float lam, const float *logits, const float *insT, const float *E,
                           float *out, hipStream_t s);
hipError_t gen_correct_bwd(int b, int n, int c, float lam, const float *logits, const float *insT, const float *E,
                           const float *grad_out, float *grad_logits, float *grad_insT, float *grad_E, hipStream_t s);

} // namespace geot
