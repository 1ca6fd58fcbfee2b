// stack_inst.hip - the explicit instantiations of launch_one (stack_kernels.h) for one raw dtype, one calibration flag and one
// group of slot counts (the table in stack_calibrate.h).  Compiled once per combination (_build.py) with
//   -DAPGPU_INST_RAW=float|uint16_t  -DAPGPU_INST_CALIB=true|false  -DAPGPU_INST_GROUP=<the group's letter>
#define APGPU_STACK_INSTANTIATE
#include "stack_kernels.h"
namespace apgpu_stack {
#define APGPU_INST_SLOTS_(GROUP) APGPU_SLOTS_##GROUP
#define APGPU_INST_SLOTS(GROUP) APGPU_INST_SLOTS_(GROUP)
#define APGPU_INSTANTIATE(NP) template int launch_one<NP, APGPU_INST_RAW, APGPU_INST_CALIB>(const StackParams &, bool, hipStream_t, char *);
APGPU_INST_SLOTS(APGPU_INST_GROUP)(APGPU_INSTANTIATE)
}
