// dX in the maps' own 16-bit dtype (offk_off_units_backward_feats_typed): the bf16 / fp16 epilogue forms of the units_dx.hip body
// (NCHW / NHWC x bf16 / fp16) and their launcher, in a code object of their own.  The kernel text is units_dx.hip's -- one body, so
// that everything up to the accumulators is the fp32 kernel's own -- but the instantiations do not share its object, so the fp32
// forms keep the code they have.
#define OFFK_UNITS_DX_F16 1
#include "units_dx.hip"
