// Q3 instantiations of the fused Helmholtz kernel (see helmholtz.hip).
#define HH_DEGREE 3
#include "helmholtz.hip"
