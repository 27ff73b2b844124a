// pow10_dd (mdns_pow10.h: the 10 ** v that host and device compute identically) over an array, for the numpy statement
// of the table model's line-of-sight effects (massivedatans_amd/tablemodel.py; mdns.h Part 12).  Compiled like every
// host file of the product: no contraction, the header's own fma() calls remain.
#include "mdns_pow10.h"

extern "C" void mdns_host_pow10_dd(const double *v, long long n, double *out)
{
	for (long long i = 0; i < n; i++) out[i] = mdns_pow10::pow10_dd(v[i]);
}
