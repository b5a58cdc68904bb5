// flow_bank.hpp -- OpticalFlowBank, the many-camera counterpart of OpticalFlowOpenCV.
//
// One object serves n_streams cameras of one frame size: what n_streams OpticalFlowOpenCV objects
// would compute frame by frame, one push() per tick computes in one device launch (the stream bank
// of include/aof.h), and the messages the reference's loop would send for that tick
// (/root/reference/src/mainloop.cpp:322-373) come back as one dense, ordered list (the bank's outbox).
// Per stream, the pushes in which it has an entry, with their quality, dt_us, flow_x and flow_y, are
// exactly the calcFlow() calls of an OpticalFlowOpenCV object, fed the same frames and (uint32_t) times,
// that return >= 0, with their outputs.  The cameras need not be alike: the constructor's focal lengths and
// output rate are every stream's starting values, and the setStream...() calls give one stream its own --
// stream s then equals an OpticalFlowOpenCV(fx_s, fy_s, rate_s, ...) object.  C++11, no exceptions; every
// host wait is bounded.
#pragma once

#include <cstdint>

struct aof_outbox_entry;   // include/aof.h: stream, MAVLink frame, tick record (quality, dt_us, flow_x, flow_y, gyro sums)
struct aof_gyro;           // include/aof.h: gyro angles integrated over the interval that ends at a frame
struct aof_exposure_command;   // include/aof.h: what the auto-exposure controller decided for a stream in a tick
struct aof_bank_stream;        // include/aof.h: one stream's focal lengths, output rate, time offset and MAVLink identity
struct aof_warp_point;         // include/aof.h: a node of a stream's warp mesh, a sensor-plane coordinate in 1/32 pixel
struct aof_field_params;       // include/aof.h: the motion-field fit's parameters (blocks needed, passes, reach, gate)
struct aof_field;              // include/aof.h: one pair's fit -- zoom, rotation, flow at the frame centre
struct aof_bank_field_record;  // include/aof.h: a stream's motion field integrated over the rate limiter's window

class OpticalFlowBank {
public:
	// The engine is configured exactly as OpticalFlowOpenCV configures itself for this frame size
	// (getPyramidLevels() says whether two levels run).  Like the other classes the constructor cannot
	// fail: without a gfx950 device the object stays alive, push() returns -1 and lastError() says why.
	OpticalFlowBank(float f_length_x, float f_length_y, int output_rate, int img_width, int img_height,
			int n_streams);
	~OpticalFlowBank();

	// The MAVLink time offset (vehicle time of time stamp 0, mainloop.cpp:360).  0, the initial value: the
	// entries carry their records and no MAVLink frame (mainloop.cpp:353-357).  Sets every stream's offset.
	void setTimestampOffset(uint64_t offset_usec);

	// What belongs to ONE camera and its vehicle (the reference takes these per process from its command line):
	// stream s's focal lengths in pixels (> 0), its output rate (<= 0 publishes every frame; the limiter's sums
	// stay as they stand, the new period applies from the next push on), the system id, component id and first
	// sequence number of its MAVLink frames, and its time offset (0: records and no frame for this stream;
	// ignored once enableImu() is on, as setTimestampOffset() is).  Each takes effect with the next push and
	// returns 0, or -EINVAL for a bad stream index (or a focal length that is not > 0), the object unchanged.
	// An object on which none of them was called runs exactly as one without them.  With enableImu() the frames
	// carry each stream's identity.
	int setStreamFocalLength(int stream, float f_length_x, float f_length_y);
	int setStreamOutputRate(int stream, int output_rate);
	int setStreamIdentity(int stream, uint8_t system_id, uint8_t component_id, uint8_t first_seq);
	int setStreamTimestampOffset(int stream, uint64_t offset_usec);

	// One tick.  frames: host memory, stream s's img_width x img_height grey frame at s * img_width *
	// img_height; img_time_us: [n_streams], the limiter sees (uint32_t)t; active: [n_streams], non-zero =
	// the stream has a frame in this tick, NULL = all; gyro: [n_streams] or NULL (zeros).  The caller may
	// release all four as soon as the call returns.  Returns the number of entries published() holds, or
	// a negative value: the engine is missing or failed, or the device did not answer within two seconds
	// (then the object has failed for good: every later push() returns a negative value at once).
	int push(const uint8_t *frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro);
	// The entries of the last push(), in stream order; valid until the next push().
	const aof_outbox_entry *published() const;
	// Masked streams (mask[s] != 0; NULL = all) start over: no previous frame, limiter and gyro sums zero,
	// the exposure gate open; with enableImu() their IMU state starts over as well, with its offset0, and the
	// samples pushImu() queued for them are dropped.  The
	// auto-exposure controllers keep what they hold: the cameras keep running.
	// This class has no call that restarts one stream's controller or overwrites its state (after a camera
	// refused a value, say): a host that needs that drives aof_bank_exposure_reset_device and a state array
	// of its own through include/aof.h.
	int reset(const uint8_t *mask);

	// The sensor-frame form: what mainloop.cpp's camera_callback does in front of calcFlow() (crop, exposure
	// statistics at 5 Hz, the auto-exposure PID of mainloop.cpp:222-271) moves behind pushCamera() for every
	// stream.  enableCamera() sizes the device memory for n_streams sensor frames of camera_width x
	// camera_height (centre-cropped to the image size), starts every controller from exposure0 / gain0 and
	// starts every stream over; exposure_interval_us: mainloop.cpp:274.  Returns 0, or a negative value:
	// -EINVAL for a second call or a sensor size that cannot hold the image (refused: the object is as it
	// was, lastError() says why), anything else for no memory or a device that did not answer (the object
	// has failed).
	int enableCamera(int camera_width, int camera_height, uint16_t exposure0, uint8_t gain0,
			 uint32_t exposure_interval_us = 200000);
	// One tick on sensor frames: stream s's frame at s * camera_width * camera_height; everything else, and
	// the return value and published(), as push().  Runs camera push, exposure control and collect on the
	// object's stream.  Needs enableCamera().
	int pushCamera(const uint8_t *sensor_frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro);
	// What belongs to ONE camera in front of the crop (include/aof.h, "per-stream sensors"): where stream s's frame lies
	// in the bytes pushCamera() takes (offset), how far apart its rows are (pitch, >= width: a V4L2 bytesperline), the
	// size of its grey plane and the origin of the image-sized crop inside it -- cameras of different resolutions, padded
	// rows, a crop around the principal point, the Y plane of a YUV420 buffer.  pushCamera() keeps taking n_streams *
	// camera_width * camera_height bytes, laid out as the records say; streams without a call keep enableCamera()'s
	// layout.  Valid after enableCamera(), from the next pushCamera() on.  Returns 0, or -EINVAL for a bad stream
	// index, without enableCamera(), or for a record that does not lie inside those bytes (the object unchanged).  An
	// object on which it was never called runs exactly as one without it.
	int setStreamSensor(int stream, uint64_t offset, int pitch, int width, int height, int x0, int y0);
	// Packed 16-bit sensor pixels (include/aof.h, "packed sensor pixels"; format: AOF_PIXEL_GREY8, _LUMA16_LO for YUYV /
	// Y16_BE, _LUMA16_HI for UYVY / Y16): the buffer a V4L2 driver filled goes in as it is, the crop takes the grey byte of
	// every pixel.  Raw mono pixels ("raw mono pixels" there; AOF_PIXEL_Y10, _Y12, _Y14, _Y10P, _Y12P) go in the same way:
	// the grey value is the top eight bits of a sample.  enableCameraPacked() is enableCamera() for cameras that all
	// deliver `format`: with row_bytes = aof_bank_pixel_row_bytes(format, camera_width) it sizes for n_streams *
	// camera_height * row_bytes bytes, every stream starts from the centred record (x0 on a pixel group) with pitch =
	// row_bytes and that format, and pushCamera() then takes that many bytes.  -EINVAL also for a value that is no format
	// (3, above 8) and for a camera_width that is not whole pixel groups of the format.
	int enableCameraPacked(int camera_width, int camera_height, int format, uint16_t exposure0, uint8_t gain0,
			       uint32_t exposure_interval_us = 200000);
	// One stream's own format, after either enable call, from the next pushCamera() on: its current record (setStreamSensor(),
	// or the enable call's) is checked again, with the new format, against the bytes pushCamera() takes; setStreamSensor()
	// checks with the stream's current format.  Returns 0, or -EINVAL, the object unchanged: a bad stream index, a value
	// that is no format, a record that no longer fits, a call before enabling.  An object on which neither call was made runs exactly
	// as before.
	int setStreamPixelFormat(int stream, int format);
	// One stream's binning (include/aof.h, "binned sensor pixels"; bin: 1, 2 or 4), after either enable call, from the next
	// pushCamera() on: a pixel of the stream's image is the rounded mean of bin x bin sensor pixels, and the crop's
	// footprint is bin * image size at the record's (x0, y0).  The stream keeps its layout, record and format; the record is
	// checked again, with the new bin, against the bytes pushCamera() takes, and setStreamSensor() and
	// setStreamPixelFormat() check with the stream's current bin.  A binned pixel subtends bin sensor pixels: the caller
	// sets focal / bin with setStreamFocalLength().  Returns 0, or -EINVAL, the object unchanged: a bad stream index, a
	// bin that is none of 1, 2, 4, a footprint that no longer fits, a call before enabling.  An object on which it was never
	// called binds nothing.
	int setStreamBinning(int stream, int bin);
	// One stream's lens (include/aof.h, "the stream bank with a lens"), after either enable call, from the next pushCamera()
	// on: the stream's image is its sensor plane resampled through a mesh of one node every 8 image pixels -- mesh:
	// aof_warp_point [ny][nx] of aof_warp_mesh_size() for the image size, sensor-plane coordinates in 1/32 pixel, copied
	// before the call returns; NULL: the stream is not warped any more (its plain crop).  The plane is the stream's record's
	// (setStreamSensor(), or the enable call's), which must stay valid as before: that rule alone refuses a frame.
	// setStreamLens() builds the mesh from the sensor camera (fx, fy, cx, cy in plane pixels) and its Brown-Conrady
	// coefficients (OpenCV's order), for a virtual pinhole camera of the same focal lengths whose principal point is the
	// image centre: the image's focal lengths are then fx, fy (setStreamFocalLength() is the caller's, as with binning).
	// A push with any stream warped still takes the one-launch tick where the library chooses it (the tick kernel with the
	// warp inside it; lastPushPath() says what the last push took).  Returns 0, or -EINVAL,
	// the object unchanged: a bad stream index, a call before enabling, focal lengths that are zero or not finite, an
	// object that bins a stream (setStreamBinning() was called: the two do not compose; setStreamBinning() refuses the
	// same way once a stream was warped).  An object on which neither was called binds nothing.
	int setStreamWarp(int stream, const aof_warp_point *mesh);
	int setStreamLens(int stream, double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double k3);
	// The last pushCamera()'s aof_exposure_command [n_streams] in pinned memory (flags 0: the stream's frame
	// was not due); valid until the next push.  NULL without enableCamera().
	const aof_exposure_command *exposureCommands() const;

	// The IMU form: what mainloop.cpp's highres_imu_msg_callback and the gates behind calcFlow() do (the gyro
	// integrator of :383-405, the stale-gyro drop of :336-342, "no vehicle time yet" of :353-357) moves behind
	// push() and pushCamera() for every stream (aof_bank_imu_device, include/aof.h).  enableImu() allocates the
	// per-stream state and a pinned staging area of max_samples (1..AOF_IMU_SLOTS_MAX) samples per stream and
	// tick, and starts every stream over; offset0: the vehicle-time offset of every stream, 0 = each stream learns
	// it from its first sample (setTimestampOffset() is not consulted any more).  From then on push() and
	// pushCamera() ignore their gyro argument, and published() holds only the records the reference would have
	// sent, their gyro sums integrated sample by sample.  Returns 0, or a negative value: -EINVAL for a second
	// call or a bad max_samples (refused: the object is as it was), anything else as enableCamera().
	int enableImu(int max_samples, uint64_t offset0 = 0);
	// Queues one HIGHRES_IMU sample (time in microseconds, rates in rad/s) for the stream's next tick.  Returns
	// 0; -ENOBUFS, the object unchanged, when the stream already holds max_samples; -EINVAL for a bad stream
	// index or without enableImu().
	int pushImu(int stream, uint64_t time_usec, float xgyro, float ygyro, float zgyro);

	// The receive path behind enableImu(): what mavlink_tcp.cpp:100-129 does with the autopilot's byte stream
	// (mavlink_parse_char byte by byte, HIGHRES_IMU decoded) moves behind push() and pushCamera() for every stream
	// (aof_bank_mavlink_rx_device, include/aof.h: the written contract of the parser).  enableMavlinkRx() allocates
	// the per-stream receive state and a pinned staging buffer of max_bytes (16..AOF_MAVLINK_RX_BYTES_MAX, a multiple
	// of 16) per stream and tick; samples queued by pushImu() are dropped.  From then on a push runs receive, tick,
	// IMU call, (exposure control,) collect on the object's stream, a frame cut by the end of a tick's bytes is
	// completed by the next tick's, and pushImu() answers -EINVAL.  A tick keeps the first max_samples samples of a
	// stream (the receive state counts the others as overflowed).  reset() also drops a masked stream's half-received
	// frame and queued bytes.  Returns 0, or a negative value: -EINVAL without enableImu(), for a second call or a
	// bad max_bytes (refused: the object is as it was), anything else as enableCamera().
	int enableMavlinkRx(int max_bytes);
	// Appends n bytes a stream's connection received (any cut of the byte stream) to its slot for the next tick.
	// Returns 0; -ENOBUFS, the object unchanged, when the slot cannot hold n more bytes; -EINVAL for a bad stream
	// index, a negative n, NULL bytes or without enableMavlinkRx().
	int pushMavlink(int stream, const uint8_t *bytes, int n);

	// The motion field (include/aof.h, "the stream bank's motion field"): zoom, rotation and the flow at the frame
	// centre, fitted to every pair's block records and integrated per stream over the rate limiter's window -- one
	// field per published message, for the camera that climbs or yaws.  enableField() allocates the per-stream state
	// and the pinned result arrays and starts every stream's window over; fp: the fit's parameters, NULL =
	// aof_field_params_default().  From then on push() and pushCamera() run aof_bank_field_device right behind the
	// bank push (in front of the IMU call: it sees the limiter's own verdicts), and reset() starts the masked
	// streams' windows over with the streams.  An object on which it was never called runs exactly as before.
	// Returns 0, or a negative value: -EINVAL for a second call, for parameters outside their ranges or for an image
	// size the fit does not serve (refused: the object is as it was), anything else as enableCamera().
	int enableField(const aof_field_params *fp = 0);
	// The last push's aof_bank_field_record [n_streams] (status >= 0: published with that many valid fits in the
	// window; AOF_TICK_HELD, AOF_TICK_IDLE, AOF_TICK_BAD_SENSOR otherwise) and the last push's own per-pair fits,
	// aof_field [n_streams] (all zero for a stream that ran no pair), in pinned memory; valid until the next push.
	// NULL without enableField().
	const aof_bank_field_record *fieldRecords() const;
	const aof_field *fields() const;

	inline int getStreams() const { return n_streams; }
	inline int getImageWidth() const { return image_width; }
	inline int getImageHeight() const { return image_height; }
	int getPyramidLevels() const;
	// How the engine ran the last accepted push()/pushCamera(): 0 none yet, 1 one launch per tick, 2 the composed
	// launches (aof_bank_last_path, include/aof.h).
	int lastPushPath() const;
	bool engineOk() const;
	const char *lastError() const;

private:
	OpticalFlowBank(const OpticalFlowBank &);
	OpticalFlowBank &operator=(const OpticalFlowBank &);
	int fail(int code, const char *what);
	int refuse(int code, const char *what);

	int image_width, image_height, n_streams;
	struct Impl;
	Impl *_m;   // engine context, device and pinned memory, stream; NULL without an engine
	bool _failed;
	char _err[200];
};
