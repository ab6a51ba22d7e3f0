// The cosine cutoff of the descriptor network (include/htf_bp.h), written once for the forces (desc_row.h) and the
// force-matching sweep (dtrain_row.h), so that the prediction and its gradient cannot drift apart.
#ifndef HTF_BP_CUTOFF_H_
#define HTF_BP_CUTOFF_H_
#include "htf_common.h"

namespace htf {
namespace {

// c_fc of cutoff_terms: fc'(r) = c_fc sin(pi r / rc)
__device__ __forceinline__ float cutoff_slope(float rc) { return -0.5f * (3.14159265358979323846f / rc); }

// fc(r) = 0.5 (cos(pi r / rc) + 1) and fc'(r) at one live distance r < rc.  sincospif: the reduction of r / rc in [0, 1) is exact.
__device__ __forceinline__ void cutoff_terms(float r, float rc, float c_fc, float &fc, float &dfc) {
    float s, c;
    sincospif(r / rc, &s, &c);
    fc = 0.5f * (c + 1.0f);
    dfc = c_fc * s;
}

} // namespace
} // namespace htf
#endif // HTF_BP_CUTOFF_H_
