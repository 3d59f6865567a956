/* Name mapping only: the device-side cuRAND header, spelled as hipRAND's.  TEST INFRASTRUCTURE ONLY. */
#pragma once
#include <hiprand/hiprand_kernel.h>
