// The owners of csrc/mdns_internal.h (DeviceBuffer, PinnedBuffer, all_or_none) on the host alone: a stand-alone program
// with the four functions of the allocation seam over malloc, a count of live blocks and a "fail the k-th call" knob.
// tests/test_owners_host.py builds it with the address and undefined-behaviour sanitizers and runs it: a block freed
// twice, leaked, or smaller than its cap() says ends the run with a report.  Exit status 0: every check held.
#include "mdns_internal.h"

#include <cstdio>
#include <cstdlib>
#include <map>

namespace {
int g_calls = 0, g_fail_at = 0;            // seam calls that can fail so far; which of them fails (0: none)
int g_frees = 0, g_errors = 0, g_drains = 0;
size_t g_last_bytes = 0;
unsigned g_last_flags = 0;
std::map<void *, size_t> g_live;           // block -> bytes

bool refused()
{
	if (++g_calls != g_fail_at) return false;
	mdns::set_error("call %d refused", g_calls);
	return true;
}
void fail_call(int k) { g_calls = 0; g_fail_at = k; }

void *take(void *old, size_t bytes, bool host)
{
	if (old) { g_drains++; mdns::scratch_free(old, host); }      // (the library waits for its stream here)
	if (refused()) return nullptr;
	void *p = malloc(bytes);
	g_live[p] = bytes;
	g_last_bytes = bytes;
	return p;
}
}  // namespace

namespace mdns {
void set_error(const char *, ...) { g_errors++; }
void *device_regrow(void *old, size_t bytes, bool zero)
{
	void *p = take(old, bytes, false);
	if (p) memset(p, zero ? 0 : 0xa5, bytes);
	return p;
}
void *pinned_regrow(void *old, size_t bytes, unsigned flags)
{
	void *p = take(old, bytes, true);
	if (p) { memset(p, 0xa5, bytes); g_last_flags = flags; }
	return p;
}
void scratch_free(void *p, bool)
{
	if (!g_live.erase(p)) { fprintf(stderr, "a block that is not live was freed\n"); exit(1); }
	g_frees++;
	free(p);
}
void *scratch_dev_pointer(void *host_block) { return refused() ? nullptr : host_block; }
}  // namespace mdns

using namespace mdns;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static constexpr unsigned kMapped = hipHostMallocMapped, kPolled = hipHostMallocMapped | hipHostMallocCoherent;

// every element of the block can be written (a block smaller than cap() says is the sanitizer's to report)
template <class T> static void touch(const DeviceBuffer<T> &b) { for (size_t i = 0; i < b.cap(); i++) b.get()[i] = T(); }

static void exact_and_grown()
{
	DeviceBuffer<double> b;
	CHECK(b.get() == nullptr && b.cap() == 0);
	CHECK(b.make(342) && b.cap() == 342 && g_last_bytes == 342 * sizeof(double));      // no half again, no page rounding
	touch(b);
	CHECK(b.make(0) && b.cap() == 1 && g_last_bytes == sizeof(double) && g_live.size() == 1);      // one element at least
	CHECK(b.make(3, true) && b.cap() == 3 && b.get()[0] == 0 && b.get()[2] == 0);
	// fit keeps its policy: half as much again in whole pages, and no call while the block is large enough
	DeviceBuffer<double> s;
	CHECK(s.fit(342) && g_last_bytes == 8192 && s.cap() == 1024);
	touch(s);
	const int calls = g_calls;
	double *const was = s.get();
	CHECK(s.fit(1024) && s.get() == was && g_calls == calls);
	CHECK(s.fit(1025) && g_last_bytes == grown_bytes(1025, 8) && s.cap() == grown_bytes(1025, 8) / 8 && g_live.size() == 2);
	CHECK(s.fit_zeroed(1) && s.cap() == grown_bytes(1025, 8) / 8);
	// make on a block that exists: stream drained, old block freed, then the exact one
	const int drains = g_drains, frees = g_frees;
	CHECK(s.make(5) && s.cap() == 5 && g_drains == drains + 1 && g_frees == frees + 1 && g_live.size() == 2);
	PinnedBuffer p;
	CHECK(p.make(100) && p.cap() == 100 && g_last_bytes == 100 && g_last_flags == hipHostMallocDefault && p.dev() == nullptr);
	for (size_t i = 0; i < p.cap(); i++) CHECK(p.get()[i] == 0);                    // zero-filled
	CHECK(p.make(0) && p.cap() == 1);
	CHECK(p.fit(4097) && p.cap() == grown_bytes(4097, 1) && p.cap() == 8192);
	PinnedBuffer m(kPolled);
	CHECK(m.make(24) && m.cap() == 24 && g_last_flags == kPolled && m.dev() == m.get());
}

static void failures_leave_nothing()
{
	const int errors = g_errors;
	DeviceBuffer<int> b;
	fail_call(1);
	CHECK(!b.make(10) && b.get() == nullptr && b.cap() == 0 && g_errors == errors + 1 && g_live.empty());
	fail_call(0);
	CHECK(b.make(10) && b.cap() == 10);
	fail_call(1);                                        // on a block that exists: the old one is gone, the buffer empty
	CHECK(!b.make(20) && b.get() == nullptr && b.cap() == 0 && g_live.empty());
	// a mapped block whose device address cannot be had ends empty, whichever of its two calls fails
	for (int k = 1; k <= 2; k++) {
		PinnedBuffer m(kMapped);
		fail_call(k);
		CHECK(!m.make(64) && m.get() == nullptr && m.dev() == nullptr && m.cap() == 0 && g_live.empty());
		fail_call(k);
		CHECK(!m.fit(64) && m.get() == nullptr && m.dev() == nullptr && m.cap() == 0 && g_live.empty());
		fail_call(0);
		CHECK(m.make(64) && m.dev() && m.cap() == 64);
	}
	CHECK(g_live.empty());
}

static void moves_free_once()
{
	fail_call(0);
	DeviceBuffer<double> a, b;
	CHECK(a.make(4) && b.make(8));
	double *const pb = b.get();
	int frees = g_frees;
	a = std::move(b);                                    // a's old block goes, exactly once
	CHECK(g_frees == frees + 1 && a.get() == pb && a.cap() == 8 && b.get() == nullptr && b.cap() == 0 && g_live.size() == 1);
	DeviceBuffer<double> c(std::move(a));
	CHECK(g_frees == frees + 1 && c.get() == pb && c.cap() == 8 && a.get() == nullptr && a.cap() == 0 && g_live.size() == 1);
	a = std::move(b);                                    // empty into empty: nothing happens
	CHECK(g_frees == frees + 1 && g_live.size() == 1);
	c = std::move(c);                                    // onto itself: kept
	CHECK(c.get() == pb && g_frees == frees + 1);

	PinnedBuffer p(kMapped), q;                          // the flags travel with the block
	CHECK(p.make(32) && q.make(16));
	char *const pp = p.get();
	frees = g_frees;
	q = std::move(p);
	CHECK(g_frees == frees + 1 && q.get() == pp && q.dev() == pp && q.cap() == 32 && p.get() == nullptr && p.dev() == nullptr && p.cap() == 0);
	PinnedBuffer r(std::move(q));
	CHECK(g_frees == frees + 1 && r.get() == pp && r.dev() == pp && r.cap() == 32 && q.get() == nullptr && g_live.size() == 2);
	CHECK(r.make(8) && g_last_flags == kMapped && r.dev() == r.get());      // (made again: still mapped)
}

// a lazily made group as the handles make theirs: a mapped mailbox and three device blocks, the last one zeroed
struct Group {
	PinnedBuffer box{kMapped};
	DeviceBuffer<double> props;
	DeviceBuffer<int> counts, ticket;
	bool make() { return all_or_none(box.make(256) && props.make(1024) && counts.make(128) && ticket.make(1, true), box, props, counts, ticket); }
	bool empty() const { return !box.get() && !box.dev() && !box.cap() && !props.get() && !counts.get() && !ticket.get() && !ticket.cap(); }
};

static void groups_are_all_or_none()
{
	Group g;
	for (int k = 1; k <= 5; k++) {                       // its five calls: block, device address, three device blocks
		fail_call(k);
		CHECK(!g.make() && g.empty() && g_live.empty());
	}
	fail_call(6);                                        // (there is no sixth)
	CHECK(g.make() && !g.empty() && g_live.size() == 4 && g_calls == 5);
	CHECK(g.box.cap() == 256 && g.props.cap() == 1024 && g.counts.cap() == 128 && g.ticket.cap() == 1 && g.ticket.get()[0] == 0);
	fail_call(0);
	Group h;                                             // the retry after a failure
	fail_call(3);
	CHECK(!h.make() && h.empty());
	fail_call(0);
	CHECK(h.make() && g_live.size() == 8);
	DeviceBuffer<int> lone;
	CHECK(all_or_none(true, lone) && !all_or_none(false, lone));
}

int main()
{
	exact_and_grown();
	CHECK(g_live.empty());
	failures_leave_nothing();
	moves_free_once();
	CHECK(g_live.empty());
	groups_are_all_or_none();
	CHECK(g_live.empty());                               // at exit nothing is live
	printf("owners ok: %d seam calls freed %d blocks\n", g_calls, g_frees);
	return 0;
}
