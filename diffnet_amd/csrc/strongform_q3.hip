// Q3 instantiations of the fused strong-form least-squares kernel (see strongform.hip).
#define SF_DEGREE 3
#include "strongform.hip"
