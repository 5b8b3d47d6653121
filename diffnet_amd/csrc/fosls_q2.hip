// Q2 instantiations of the fused first-order-system least-squares kernel (see fosls.hip).
#define FO_DEGREE 2
#include "fosls.hip"
