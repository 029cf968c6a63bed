// Stand-in for <cuda.h> (the driver API header): the reference's kernel
// headers include it and use nothing from it.
#pragma once
#include <cuda_runtime.h>
