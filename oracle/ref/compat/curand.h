/* Name mapping only: the cuRAND host names RandGenGPU / op_uniform_init use, spelled as hipRAND's.  Nothing the
 * driver instantiates draws a random number, so the program links without the hipRAND library.
 * TEST INFRASTRUCTURE ONLY. */
#pragma once
#include <hiprand/hiprand.h>

#define curandStatus_t hiprandStatus_t
#define CURAND_STATUS_SUCCESS HIPRAND_STATUS_SUCCESS
#define curandGenerator_t hiprandGenerator_t
#define CURAND_RNG_PSEUDO_DEFAULT HIPRAND_RNG_PSEUDO_DEFAULT
#define curandCreateGenerator hiprandCreateGenerator
#define curandSetPseudoRandomGeneratorSeed hiprandSetPseudoRandomGeneratorSeed
#define curandGenerateUniform hiprandGenerateUniform
