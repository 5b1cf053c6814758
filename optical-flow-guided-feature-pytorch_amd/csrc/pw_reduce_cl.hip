// K1 on channels-last bf16 / fp16 feature maps (offk_pw_reduce_cl, offk_off_units_cl, offk_off_units_train_cl): the channels-last
// 16-bit instantiations of pw_reduce_kernel and their launcher, in a code object of their own for the reason pw_reduce_f16.hip
// gives: the existing forms keep the register allocation they have.  (fp32 channels-last maps run the fp32 forms' mode 2.)
#define OFFK_PW_REDUCE_CL16 1
#include "pw_reduce.hip"
