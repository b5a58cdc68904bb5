// flow_bank.hpp -- OpticalFlowBank, the many-camera counterpart of OpticalFlowOpenCV.
//
// One object serves n_streams cameras of one frame size: what n_streams OpticalFlowOpenCV objects
// would compute frame by frame, one push() per tick computes in one device launch (the stream bank
// of include/aof.h), and the messages the reference's loop would send for that tick
// (/root/reference/src/mainloop.cpp:322-373) come back as one dense, ordered list (the bank's outbox).
// Per stream, the pushes in which it has an entry, with their quality, dt_us, flow_x and flow_y, are
// exactly the calcFlow() calls of an OpticalFlowOpenCV object, fed the same frames and (uint32_t) times,
// that return >= 0, with their outputs.  C++11, no exceptions; every host wait is bounded.
#pragma once

#include <cstdint>

struct aof_outbox_entry;   // include/aof.h: stream, MAVLink frame, tick record (quality, dt_us, flow_x, flow_y, gyro sums)
struct aof_gyro;           // include/aof.h: gyro angles integrated over the interval that ends at a frame

class OpticalFlowBank {
public:
	// The engine is configured exactly as OpticalFlowOpenCV configures itself for this frame size
	// (getPyramidLevels() says whether two levels run).  Like the other classes the constructor cannot
	// fail: without a gfx950 device the object stays alive, push() returns -1 and lastError() says why.
	OpticalFlowBank(float f_length_x, float f_length_y, int output_rate, int img_width, int img_height,
			int n_streams);
	~OpticalFlowBank();

	// The MAVLink time offset (vehicle time of time stamp 0, mainloop.cpp:360).  0, the initial value: the
	// entries carry their records and no MAVLink frame (mainloop.cpp:353-357).
	void setTimestampOffset(uint64_t offset_usec);

	// One tick.  frames: host memory, stream s's img_width x img_height grey frame at s * img_width *
	// img_height; img_time_us: [n_streams], the limiter sees (uint32_t)t; active: [n_streams], non-zero =
	// the stream has a frame in this tick, NULL = all; gyro: [n_streams] or NULL (zeros).  The caller may
	// release all four as soon as the call returns.  Returns the number of entries published() holds, or
	// a negative value: the engine is missing or failed, or the device did not answer within two seconds
	// (then the object has failed for good: every later push() returns a negative value at once).
	int push(const uint8_t *frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro);
	// The entries of the last push(), in stream order; valid until the next push().
	const aof_outbox_entry *published() const;
	// Masked streams (mask[s] != 0; NULL = all) start over: no previous frame, limiter and gyro sums zero.
	int reset(const uint8_t *mask);

	inline int getStreams() const { return n_streams; }
	inline int getImageWidth() const { return image_width; }
	inline int getImageHeight() const { return image_height; }
	int getPyramidLevels() const;
	bool engineOk() const;
	const char *lastError() const;

private:
	OpticalFlowBank(const OpticalFlowBank &);
	OpticalFlowBank &operator=(const OpticalFlowBank &);
	int fail(int code, const char *what);
	bool waitIdle();

	int image_width, image_height, n_streams;
	struct Impl;
	Impl *_m;   // engine context, device and pinned memory, stream; NULL without an engine
	bool _failed;
	char _err[200];
};
