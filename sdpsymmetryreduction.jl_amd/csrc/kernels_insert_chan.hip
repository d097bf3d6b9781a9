// Insert pass of the refinement (refine_insert.h) for the channel sources: int32 or f32 squares, 1, 2, 4 or 8 channels.
#include "refine_insert.h"

namespace sdpsr {

#define INSERT_FAMILY(X)                                                                            \
    X(SrcChan<int32_t, 1>) X(SrcChan<int32_t, 2>) X(SrcChan<int32_t, 4>) X(SrcChan<int32_t, 8>) \
    X(SrcChan<float, 1>) X(SrcChan<float, 2>) X(SrcChan<float, 4>) X(SrcChan<float, 8>)

INSERT_FAMILY(SDPSR_INSERT_INSTANTIATE)

// per-device kernel attributes, set by sdpsr_create() (see gemm_set_device_attributes)
bool insert_chan_set_device_attributes() {
    bool ok = true;
    INSERT_FAMILY(SDPSR_INSERT_MID_ATTRIBUTE)
    return ok;
}

}  // namespace sdpsr
