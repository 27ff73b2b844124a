// pow10_dd (csrc/mdns_pow10.h, the host side of the header the chain kernel includes) over an array,
// for tests/test_pow10.py and the numpy statement of the chained first batch.
#include "mdns_pow10.h"

extern "C" void pow10_dd_array(const double *v, int n, double *out)
{
	for (int i = 0; i < n; i++) out[i] = mdns_pow10::pow10_dd(v[i]);
}
