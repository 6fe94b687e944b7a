/*
 * ref_sincos.h -- force-included (-include) when src/ORBextractor.cc is compiled for ref_orbx.
 *
 * computeOrbDescriptor (src/ORBextractor.cc:115) calls cos / sin of a float from inside namespace
 * ORB_SLAM2.  Declaring ORB_SLAM2::cos(float) / sin(float) here makes unqualified lookup stop in that
 * namespace, so those two calls bind to ref_orbx.cc's definitions -- the correctly rounded fp32 values
 * the project takes as canonical -- without editing the reference.  No other
 * call in the file is affected.
 */
#ifndef ORBX_REF_SINCOS_H
#define ORBX_REF_SINCOS_H
namespace ORB_SLAM2 {
float cos(float x);
float sin(float x);
}
#endif
