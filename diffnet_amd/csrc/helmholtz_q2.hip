// Q2 instantiations of the fused Helmholtz kernel (see helmholtz.hip).
#define HH_DEGREE 2
#include "helmholtz.hip"
