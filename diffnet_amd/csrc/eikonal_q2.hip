// Q2 instantiations of the fused eikonal kernel (see eikonal.hip).
#define EK_DEGREE 2
#include "eikonal.hip"
