// Insert pass of the refinement (refine_insert.h) for the signature array and the value pairs.
#include "refine_insert.h"

namespace sdpsr {

#define INSERT_FAMILY(X) X(SrcArray) X(SrcPair)

INSERT_FAMILY(SDPSR_INSERT_INSTANTIATE)

// per-device kernel attributes, set by sdpsr_create() (see gemm_set_device_attributes)
bool insert_array_pair_set_device_attributes() {
    bool ok = true;
    INSERT_FAMILY(SDPSR_INSERT_MID_ATTRIBUTE)
    return ok;
}

}  // namespace sdpsr
