// Q2 instantiations of the fused strong-form least-squares kernel (see strongform.hip).
#define SF_DEGREE 2
#include "strongform.hip"
