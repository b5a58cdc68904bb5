// The state of one per-stream table of OpticalFlowBank (flow_bank.cpp): a shadow array in pinned memory that setters
// write, its copy on the device, and the binding of that copy to the context.  Here only the four flags and their
// transitions, which need neither the HIP runtime nor the C ABI: the copy and the binding call are the caller's
// (tests/native/host_selftest.cpp drives the same transitions with counters in their place).
//
// Nothing is copied or bound before a setter has marked the table used: without one the tick runs on the scalars, as
// it always did.  A used table is copied in front of every tick while it is dirty and bound in front of the first.
// The shadow counts as copied only once the tick's tag has been seen (tagSeen()): a push that fails between the copy
// and the collect leaves the table dirty, so the next tick copies again -- and a setter behind such a push writes an
// array that is still marked dirty.
#pragma once

struct BankTableFlags {
	bool used;      // a setter has been called: the table takes part in the ticks
	bool dirty;     // the shadow holds what the device does not
	bool bound;     // the device array is bound to the context
	bool copying;   // a copy of the shadow is enqueued: it is through once the tick's tag has been seen

	void touch() { used = dirty = true; }                 // a setter changed the shadow
	void touchUnused() { dirty = true; }                  // the shadow changed, but by no per-stream setter: copied once one is called
	void rideAlong() { used = true; if (!bound) dirty = true; }   // another table's setter needs this one bound beside it

	// In front of a tick: upload() enqueues the copy, bind() binds the device array; each returns 0 or the tick's
	// failure, which is returned as it is.  The copy comes before the binding.
	template <class Upload, class Bind>
	int sync(Upload upload, Bind bind)
	{
		if (!used) return 0;
		if (dirty) {
			if (const int rc = upload()) return rc;
			copying = true;   // (still dirty: a push that fails behind this point copies again)
		}
		if (!bound) {
			if (const int rc = bind()) return rc;
			bound = true;
		}
		return 0;
	}
	// The tick's tag has been seen: the copy in front of the tick is through as well.
	void tagSeen()
	{
		if (copying) copying = dirty = false;
	}
};
