// Insert pass of the refinement (refine_insert.h) for the joint sources: projection onto r = 0 .. 4 basis matrices and
// 2 or 4 channels of the square in one signature.
#include "refine_insert.h"

namespace sdpsr {

#define INSERT_FAMILY(X)                                                                                    \
    X(SrcJoint<0, 2>) X(SrcJoint<1, 2>) X(SrcJoint<2, 2>) X(SrcJoint<3, 2>) X(SrcJoint<4, 2>) \
    X(SrcJoint<0, 4>) X(SrcJoint<1, 4>) X(SrcJoint<2, 4>) X(SrcJoint<3, 4>) X(SrcJoint<4, 4>)

INSERT_FAMILY(SDPSR_INSERT_INSTANTIATE)

// per-device kernel attributes, set by sdpsr_create() (see gemm_set_device_attributes)
bool insert_joint_set_device_attributes() {
    bool ok = true;
    INSERT_FAMILY(SDPSR_INSERT_MID_ATTRIBUTE)
    return ok;
}

}  // namespace sdpsr
