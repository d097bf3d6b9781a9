// Insert pass of the refinement (refine_insert.h) for the projection sources, r = 0 .. 4 basis matrices.
#include "refine_insert.h"

namespace sdpsr {

#define INSERT_FAMILY(X) X(SrcProj<0>) X(SrcProj<1>) X(SrcProj<2>) X(SrcProj<3>) X(SrcProj<4>)

INSERT_FAMILY(SDPSR_INSERT_INSTANTIATE)

// per-device kernel attributes, set by sdpsr_create() (see gemm_set_device_attributes)
bool insert_proj_set_device_attributes() {
    bool ok = true;
    INSERT_FAMILY(SDPSR_INSERT_MID_ATTRIBUTE)
    return ok;
}

}  // namespace sdpsr
