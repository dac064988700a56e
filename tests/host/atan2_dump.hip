// Host driver of cam_atan2_rounded (csrc/satba_camapprox.h) for tests/test_atan2_host.py: reads hex-float pairs "y x" from stdin and
// prints the result of every pair as a hex float, one per line.  It calls no HIP API and runs on a machine without a device.
#include <cstdio>
#include "satba_camapprox.h"

int main() {
    double y, x;
    while (std::scanf("%la %la", &y, &x) == 2) std::printf("%a\n", satba::cam_atan2_rounded(y, x));
    return 0;
}
