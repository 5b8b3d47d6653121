// Q3 instantiations of the fused eikonal kernel (see eikonal.hip).
#define EK_DEGREE 3
#include "eikonal.hip"
