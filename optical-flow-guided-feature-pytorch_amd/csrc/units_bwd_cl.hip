// K1b on channels-last feature maps (offk_off_units_backward_cl): the channels-last X loader instantiations of pw_wgrad_kernel
// (fp32, bf16, fp16) and their launcher, in a code object of their own.  The kernel text is units_bwd.hip's -- one template, so that
// everything behind the LDS store is the NCHW kernel's own -- but the instantiations do not share its object, so the NCHW forms
// keep the code they have.
#define OFFK_UNITS_BWD_CL 1
#include "units_bwd.hip"
