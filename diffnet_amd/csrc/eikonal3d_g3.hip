// 3-point-rule instantiations of the fused 3-D eikonal kernel (see eikonal3d.hip).
#define EK3_NGP 3
#include "eikonal3d.hip"
