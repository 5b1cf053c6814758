// K1 on bf16 / fp16 feature maps (offk_pw_reduce_typed, offk_off_units_typed, offk_off_units_train_typed): the 16-bit map
// instantiations of pw_reduce_kernel and their launcher, in a code object of their own.  The kernel text is pw_reduce.hip's --
// one template, so that everything behind the LDS store is the fp32 kernel's own -- but the instantiations do not share its
// object: with them in it, the fp32 forms came out of the compiler with a different register allocation.
#define OFFK_PW_REDUCE_FEAT16 1
#include "pw_reduce.hip"
