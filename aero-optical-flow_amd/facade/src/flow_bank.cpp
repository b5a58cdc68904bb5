// OpticalFlowBank (flow_bank.hpp): S cameras per push() through the stream bank of the C ABI and its outbox
// (aof_bank_collect_device) in pinned host memory.  Impl::tick() is one push, plain or on sensor frames, in every form:
// its body is the order of the copies and launches on the object's stream, closed by a bounded poll of the outbox's tag
// -- no stream synchronisation anywhere.  Impl::startOver() is the one way streams start over.  Every byte of device and
// pinned memory is taken through Impl::mem, which the destructor releases in one loop.
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>

#include <hip/hip_runtime_api.h>

#include "aof.h"
#include "bank_table.hpp"
#include "flow_bank.hpp"
#include "opencv_params.hpp"
#include "optical_flow_rad.hpp"

namespace {

// every host wait for the device ends after this long (a tick runs microseconds to a millisecond)
const double kDeadlineS = 2.0;

size_t alignUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

double secondsSince(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// Every allocation of one object, recorded where it is made: release() frees them all, the newest first.
struct Allocations {
	enum Kind { kDevice, kPinned, kOutbox };   // hipMalloc, hipHostMalloc, aof_outbox_alloc_host: each has its own free
	struct { void *p; Kind kind; } list[34];   // (31 with every form on, 32 inside enableCamera())
	int n;

	bool get(void **p, size_t bytes, Kind kind)
	{
		*p = NULL;
		const bool ok = n < (int)(sizeof(list) / sizeof(list[0])) &&
				(kind == kDevice   ? hipMalloc(p, bytes) == hipSuccess
				 : kind == kPinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess
						   : aof_outbox_alloc_host(bytes, p) == 0);
		if (!ok) return false;
		list[n].p = *p;
		list[n++].kind = kind;
		return true;
	}
	void freeAt(int i)
	{
		if (list[i].kind == kOutbox) aof_outbox_free_host(list[i].p);
		else if (list[i].kind == kPinned) (void)hipHostFree(list[i].p);
		else (void)hipFree(list[i].p);
	}
	void drop(void *p)   // one of them ahead of the others
	{
		for (int i = 0; i < n; i++) {
			if (list[i].p != p) continue;
			freeAt(i);
			list[i] = list[--n];
			return;
		}
	}
	void release()
	{
		while (n > 0) freeAt(--n);
	}
};

// A staging block: the same layout in pinned host memory (zeroed) and on the device.
struct Staged {
	uint8_t *h, *d;
	size_t bytes;

	bool alloc(Allocations &mem, size_t n)
	{
		bytes = n;
		if (!mem.get((void **)&h, n, Allocations::kPinned) || !mem.get((void **)&d, n, Allocations::kDevice)) return false;
		std::memset(h, 0, n);
		return true;
	}
	bool upload(hipStream_t stream, size_t offset, size_t n) const
	{
		return hipMemcpyAsync(d + offset, h + offset, n, hipMemcpyHostToDevice, stream) == hipSuccess;
	}
};

// A per-stream table: a shadow array the setters write and its copy on the device, with the flags that decide when it
// is copied and bound (bank_table.hpp).  The four of an object, in the order a tick copies and binds them.
struct Table : Staged, BankTableFlags {};
enum { kSensors, kFormats, kBins, kStreams, kWarps, kTables };
const char *const kTableCopyFailed[kTables] = {
	"copy of the per-stream sensor records failed", "copy of the per-stream pixel formats failed",
	"copy of the per-stream binning failed", "copy of the per-stream records failed", "copy of the per-stream warp meshes failed"};
// The one thing the tables differ in: the call of the C ABI that binds the device array (camera_bytes: of the sensor records).
int bindTable(aof_ctx *ctx, int which, const uint8_t *d, int n_streams, size_t camera_bytes)
{
	switch (which) {
	case kSensors: return aof_set_bank_sensors(ctx, reinterpret_cast<const aof_bank_sensor *>(d), n_streams, camera_bytes);
	case kFormats: return aof_set_bank_pixel_formats(ctx, d, n_streams);
	case kBins: return aof_set_bank_binning(ctx, d, n_streams);
	case kWarps: return aof_set_bank_warps(ctx, reinterpret_cast<const aof_warp_point *>(d), n_streams);
	default: return aof_set_bank_streams(ctx, reinterpret_cast<const aof_bank_stream *>(d), n_streams);
	}
}

}  // namespace

struct OpticalFlowBank::Impl {
	OpticalFlowBank *self;   // (for fail())
	size_t S;                // n_streams
	aof_ctx *ctx;
	aof_bank_params bp;
	hipStream_t stream;
	Allocations mem;
	Staged stage;            // frames, times, gyro, masks
	size_t off_times, off_gyro, off_active;
	void *d_bank;
	size_t bank_bytes;
	aof_tick_record *d_records;
	uint8_t *d_mavlink, *d_lens;
	uint8_t *outbox;         // pinned (aof_outbox_alloc_host): header, then n_streams entries
	size_t outbox_bytes;
	uint64_t tag;
	// the sensor-frame form (enableCamera): sensor frames staged apart from the block above
	bool camera;
	aof_bank_camera cam;
	aof_exposure_control ec;
	Staged sensor;           // all n_streams sensor frames
	aof_exposure_record *d_exposure;
	aof_exposure_state *d_exposure_state;
	aof_exposure_command *commands;    // pinned (aof_outbox_alloc_host): [n_streams]
	// the IMU form (enableImu): samples queued by pushImu() for the next tick
	bool imu;
	aof_imu_params ip;
	uint64_t imu_offset0;
	Staged samples;          // aof_imu_sample [slots][n_streams], then their counts u8 [n_streams]
	size_t off_imu_counts;
	aof_imu_state *d_imu_state;
	// the receive path (enableMavlinkRx): bytes queued by pushMavlink() for the next tick
	bool rx;
	aof_mavlink_rx_params rp;
	Staged bytes;            // u8 [n_streams][max_bytes], then their lengths u16 [n_streams]
	size_t off_rx_len;
	aof_mavlink_rx_state *d_rx_state;
	// the motion field (enableField): the fit and its window behind every push
	bool field;
	aof_field_params field_params;
	aof_bank_field_state *d_field_state;
	aof_bank_field_record *field_records;   // pinned (aof_outbox_alloc_host): [n_streams]
	aof_field *field_fits;                  // pinned (aof_outbox_alloc_host): [n_streams]
	// the per-stream tables; nothing of one is copied or bound before its first setter
	//   kStreams  (setStream...()): aof_bank_stream [n_streams], the shadow records start from the constructor's values
	//   kSensors  (setStreamSensor()): aof_bank_sensor [n_streams], allocated by enableCamera() like the next two; the
	//             shadow records start from what its sensor size means (aof_bank_sensor_from_camera)
	//   kFormats  (enableCameraPacked(), setStreamPixelFormat()): u8 [n_streams]; they travel with the sensor records
	//             (used implies that the records are)
	//   kBins     (setStreamBinning()): u8 [n_streams], ones until a call; beside the records as well
	//   kWarps    (setStreamWarp(), setStreamLens()): aof_warp_point [n_streams][mesh_nodes], allocated by enableCamera();
	//             every mesh starts unwarped (AOF_WARP_NONE in its first node); bound on its own, never beside kBins
	Table table[kTables];
	size_t mesh_nodes;       // nodes of one stream's mesh (aof_warp_mesh_size)

	int fail(int code, const char *what) { return self->fail(code, what); }
	int failed(int rc) { return rc ? fail(rc, aof_last_error(ctx)) : 0; }   // of a call of the C ABI
	uint8_t *imuCounts() { return samples.h + off_imu_counts; }
	uint16_t *rxLengths() { return reinterpret_cast<uint16_t *>(bytes.h + off_rx_len); }
	aof_bank_stream *shadow() { return reinterpret_cast<aof_bank_stream *>(table[kStreams].h); }
	aof_bank_sensor *sensorRecords() { return reinterpret_cast<aof_bank_sensor *>(table[kSensors].h); }
	aof_warp_point *mesh(int s) { return reinterpret_cast<aof_warp_point *>(table[kWarps].h) + (size_t)s * mesh_nodes; }
	static aof_warp_point *meshFor(OpticalFlowBank *self, int s);
	static aof_bank_stream *record(Impl *m, int s);
	bool waitIdle();
	int startOver(const uint8_t *mask, bool imu_too);
	int enableSensorFrames(int camera_width, int camera_height, int format, uint16_t exposure0, uint8_t gain0, uint32_t interval_us);
	int tick(bool sensor_frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro);
	int receive();
	int syncStreams();
	int takeImu();
	int collect();
};

OpticalFlowBank::OpticalFlowBank(float f_length_x, float f_length_y, int output_rate, int img_width, int img_height,
				 int streams)
	: image_width(img_width), image_height(img_height), n_streams(streams), _m(NULL), _failed(false)
{
	std::snprintf(_err, sizeof(_err), "engine not opened");
	Impl *m = new (std::nothrow) Impl();
	if (!m) return;
	aof_params p;
	opencvEngineParams(img_width, img_height, DEFAULT_NUMBER_OF_FEATURES, &p);
	int rc = streams < 1 ? -EINVAL : aof_create(&p, 0, &m->ctx);
	if (rc) {
		// as the single-camera classes: stay alive, never publish, say why once
		std::snprintf(_err, sizeof(_err), "aof_create failed: %s", streams < 1 ? "n_streams < 1" : aof_strerror(rc));
		std::fprintf(stderr, "OpticalFlowBank: %s (no CPU fallback; flow output disabled)\n", _err);
		delete m;
		return;
	}
	m->self = this;
	std::memset(&m->bp, 0, sizeof(m->bp));
	m->bp.n_streams = streams;
	m->bp.focal_x = f_length_x;
	m->bp.focal_y = f_length_y;
	m->bp.output_rate = output_rate;
	m->bp.system_id = MAVLINK_SYSTEM_ID_DEFAULT;
	m->bp.component_id = MAVLINK_COMPONENT_ID_CAMERA;
	const size_t S = m->S = (size_t)streams, frame = (size_t)img_width * img_height;
	m->off_times = alignUp(S * frame, 256);
	m->off_gyro = alignUp(m->off_times + S * sizeof(uint64_t), 256);
	m->off_active = alignUp(m->off_gyro + S * sizeof(aof_gyro), 256);
	struct aof_bank_layout L;
	struct aof_outbox_layout O;
	bool ok = aof_bank_layout(&p, &m->bp, &L) == 0 && aof_outbox_layout((uint32_t)streams, 0, &O) == 0;
	if (ok) {
		m->bank_bytes = L.total_bytes;
		m->outbox_bytes = O.total_bytes;
		ok = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) == hipSuccess &&
		     m->stage.alloc(m->mem, alignUp(m->off_active + S, 256)) &&
		     m->mem.get(&m->d_bank, m->bank_bytes, Allocations::kDevice) &&
		     m->mem.get((void **)&m->d_records, S * sizeof(aof_tick_record), Allocations::kDevice) &&
		     m->mem.get((void **)&m->d_mavlink, S * AOF_SEQ_FRAME_BYTES, Allocations::kDevice) &&
		     m->mem.get((void **)&m->d_lens, S, Allocations::kDevice) &&
		     m->table[kStreams].alloc(m->mem, S * sizeof(aof_bank_stream)) &&
		     m->mem.get((void **)&m->outbox, m->outbox_bytes, Allocations::kOutbox);
	}
	_m = m;
	if (!ok) {
		fail(-ENOMEM, "device or pinned memory for the bank could not be allocated");
		return;
	}
	std::memset(m->outbox, 0, m->outbox_bytes);
	for (size_t s = 0; s < S; s++) aof_bank_stream_from_params(&m->bp, &m->shadow()[s]);
	std::snprintf(_err, sizeof(_err), "ok");
	if (m->startOver(NULL, false)) return;
	m->waitIdle();
}

OpticalFlowBank::~OpticalFlowBank()
{
	if (!_m) return;
	Impl *m = _m;
	// a bounded wait, as everywhere: memory a kernel may still write is leaked, not freed
	if (!m->stream || m->waitIdle()) {
		m->mem.release();
		if (m->stream) (void)hipStreamDestroy(m->stream);
		if (m->ctx) aof_destroy(m->ctx);
	} else {
		std::fprintf(stderr, "OpticalFlowBank: the device did not drain: its memory is leaked, not freed\n");
	}
	delete m;
}

int OpticalFlowBank::fail(int code, const char *what)
{
	_failed = true;
	std::snprintf(_err, sizeof(_err), "%s", what);
	return code;
}

// A refused call: lastError() says why, the object stays usable.
int OpticalFlowBank::refuse(int code, const char *what)
{
	std::snprintf(_err, sizeof(_err), "%s", what);
	return code;
}

// The object's stream has nothing left to do (polled, with the deadline); false fails the object.
bool OpticalFlowBank::Impl::waitIdle()
{
	const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	for (;;) {
		const hipError_t e = hipStreamQuery(stream);
		if (e == hipSuccess) return true;
		if (e != hipErrorNotReady) {
			fail(-EIO, hipGetErrorString(e));
			return false;
		}
		if (secondsSince(t0) > kDeadlineS) {
			fail(-ETIMEDOUT, "the device did not finish within the deadline");
			return false;
		}
	}
}

// Masked streams (mask[s] != 0; NULL: all) start over, enqueued on the object's stream: their part of the bank, their
// IMU state if the form is on (imu_too: or is being turned on), their receive state and the window of their motion field
// if those are on.  What the pinned
// queues hold for them belongs to their past and is dropped with it.  The caller waits (waitIdle()).
int OpticalFlowBank::Impl::startOver(const uint8_t *mask, bool imu_too)
{
	const uint8_t *d_mask = NULL;
	if (mask) {
		std::memcpy(stage.h + off_active, mask, S);
		if (!stage.upload(stream, off_active, S)) return fail(-EIO, "copy of the reset mask failed");
		d_mask = stage.d + off_active;
	}
	int rc = failed(aof_bank_reset_device(ctx, &bp, d_mask, d_bank, bank_bytes, stream));
	if (!rc && imu_too) rc = failed(aof_bank_imu_reset_device(ctx, (int)S, d_mask, imu_offset0, d_imu_state, stream));
	if (!rc && rx) rc = failed(aof_bank_mavlink_rx_reset_device(ctx, (int)S, d_mask, d_rx_state, stream));
	if (!rc && field) rc = failed(aof_bank_field_reset_device(ctx, (int)S, d_mask, d_field_state, stream));
	if (rc) return rc;
	for (size_t s = 0; s < S; s++) {
		if (mask && !mask[s]) continue;
		if (imu_too) imuCounts()[s] = 0;
		if (rx) rxLengths()[s] = 0;   // (the frame half received went with the receive state)
	}
	return 0;
}

void OpticalFlowBank::setTimestampOffset(uint64_t offset_usec)
{
	if (!_m) return;
	_m->bp.offset_timestamp_usec = offset_usec;
	if (!_m->shadow()) return;
	for (int s = 0; s < n_streams; s++) _m->shadow()[s].offset_timestamp_usec = offset_usec;
	_m->table[kStreams].touchUnused();
}

// The shadow record of stream s for a setter, or NULL (no engine, no memory, bad index); the next push copies the array.
aof_bank_stream *OpticalFlowBank::Impl::record(Impl *m, int s)
{
	if (!m || !m->shadow() || s < 0 || (size_t)s >= m->S) return NULL;
	m->table[kStreams].touch();
	return &m->shadow()[s];
}

int OpticalFlowBank::setStreamFocalLength(int s, float f_length_x, float f_length_y)
{
	if (!(f_length_x > 0.0f) || !(f_length_y > 0.0f)) return -EINVAL;
	aof_bank_stream *r = Impl::record(_m, s);
	if (!r) return -EINVAL;
	r->focal_x = f_length_x;
	r->focal_y = f_length_y;
	return 0;
}

int OpticalFlowBank::setStreamOutputRate(int s, int output_rate)
{
	aof_bank_stream *r = Impl::record(_m, s);
	if (!r) return -EINVAL;
	r->output_rate = output_rate;
	return 0;
}

int OpticalFlowBank::setStreamIdentity(int s, uint8_t system_id, uint8_t component_id, uint8_t first_seq)
{
	aof_bank_stream *r = Impl::record(_m, s);
	if (!r) return -EINVAL;
	r->system_id = system_id;
	r->component_id = component_id;
	r->first_seq = first_seq;
	return 0;
}

int OpticalFlowBank::setStreamTimestampOffset(int s, uint64_t offset_usec)
{
	if (!_m || s < 0 || s >= n_streams) return -EINVAL;
	if (_m->imu) return 0;   // (the IMU form keeps every stream's offset in its IMU state, as with setTimestampOffset())
	aof_bank_stream *r = Impl::record(_m, s);
	if (!r) return -EINVAL;
	r->offset_timestamp_usec = offset_usec;
	return 0;
}

int OpticalFlowBank::setStreamSensor(int s, uint64_t offset, int pitch, int width, int height, int x0, int y0)
{
	Impl *m = _m;
	if (!m || !m->camera || !m->sensorRecords() || s < 0 || s >= n_streams) return -EINVAL;
	aof_bank_sensor rec;
	std::memset(&rec, 0, sizeof(rec));
	rec.offset = offset;
	rec.pitch = pitch;
	rec.width = width;
	rec.height = height;
	rec.x0 = x0;
	rec.y0 = y0;
	// the kernels' own rule, against the staging buffer pushCamera() fills: here the host can see the record
	// (with the stream's current pixel format and binning)
	if (aof_bank_sensor_valid_binned(&rec, m->table[kFormats].h[s], m->table[kBins].h[s], image_width, image_height, 0, m->sensor.bytes) != 1)
		return refuse(-EINVAL, "setStreamSensor(): the record does not describe memory inside the staging buffer");
	m->sensorRecords()[s] = rec;
	m->table[kSensors].touch();
	return 0;
}

int OpticalFlowBank::setStreamPixelFormat(int s, int format)
{
	Impl *m = _m;
	if (!m || !m->camera || !m->sensorRecords() || !m->table[kFormats].h || s < 0 || s >= n_streams) return -EINVAL;
	int64_t group_row = 0;   // (a row of four pixels is whole groups of every format: this asks for the format alone)
	if (format < 0 || format > 255 || aof_bank_pixel_row_bytes((uint8_t)format, 4, &group_row))
		return refuse(-EINVAL, "setStreamPixelFormat(): no such format");
	// the stream's current record, by the kernels' own rule, with the new format
	if (aof_bank_sensor_valid_binned(m->sensorRecords() + s, (uint8_t)format, m->table[kBins].h[s], image_width,
					 image_height, 0, m->sensor.bytes) != 1)
		return refuse(-EINVAL, "setStreamPixelFormat(): the stream's record no longer lies inside the staging buffer");
	m->table[kFormats].h[s] = (uint8_t)format;
	m->table[kFormats].touch();
	m->table[kSensors].rideAlong();   // (formats are bound next to the records only)
	return 0;
}

int OpticalFlowBank::setStreamBinning(int s, int bin)
{
	Impl *m = _m;
	if (!m || !m->camera || !m->sensorRecords() || !m->table[kFormats].h || !m->table[kBins].h || s < 0 || s >= n_streams) return -EINVAL;
	if (bin != 1 && bin != 2 && bin != 4) return refuse(-EINVAL, "setStreamBinning(): the bin is 1, 2 or 4");
	if (m->table[kWarps].used) return refuse(-EINVAL, "setStreamBinning(): the object warps streams (setStreamWarp()): binning and warp do not compose");
	// the stream's current record and format, by the kernels' own rule, with the new footprint
	if (aof_bank_sensor_valid_binned(m->sensorRecords() + s, m->table[kFormats].h[s], (uint8_t)bin, image_width,
					 image_height, 0, m->sensor.bytes) != 1)
		return refuse(-EINVAL, "setStreamBinning(): the binned crop no longer lies inside the stream's sensor frame");
	m->table[kBins].h[s] = (uint8_t)bin;
	m->table[kBins].touch();
	m->table[kSensors].rideAlong();   // (the binning is bound next to the records only)
	return 0;
}

// Stream s's shadow mesh for a setter, or NULL (refused: not enabled, a bad index, a binning in use); the next
// pushCamera() copies the array.
aof_warp_point *OpticalFlowBank::Impl::meshFor(OpticalFlowBank *self, int s)
{
	Impl *m = self->_m;
	if (!m || !m->camera || !m->table[kWarps].h || s < 0 || s >= self->n_streams) return NULL;
	if (m->table[kBins].used) {
		self->refuse(-EINVAL, "setStreamWarp(): the object bins streams (setStreamBinning()): binning and warp do not compose");
		return NULL;
	}
	m->table[kWarps].touch();
	return m->mesh(s);
}

int OpticalFlowBank::setStreamWarp(int s, const aof_warp_point *mesh)
{
	aof_warp_point *dst = Impl::meshFor(this, s);
	if (!dst) return -EINVAL;
	if (mesh) std::memcpy(dst, mesh, _m->mesh_nodes * sizeof(aof_warp_point));
	else dst[0].x = AOF_WARP_NONE;
	return 0;
}

int OpticalFlowBank::setStreamLens(int s, double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double k3)
{
	if (!_m || !_m->camera) return -EINVAL;
	aof_params p;
	if (aof_get_params(_m->ctx, &p)) return -EINVAL;
	const aof_lens lens = {fx, fy, cx, cy, k1, k2, p1, p2, k3, fx, fy, image_width / 2.0, image_height / 2.0};
	if (!(fx == fx) || !(fy == fy) || fx == 0.0 || fy == 0.0 || fx - fx != 0.0 || fy - fy != 0.0)
		return refuse(-EINVAL, "setStreamLens(): the focal lengths must be finite and not zero");
	aof_warp_point *dst = Impl::meshFor(this, s);
	if (!dst) return -EINVAL;
	return aof_warp_mesh_from_lens(&p, &lens, dst);
}

int OpticalFlowBank::getPyramidLevels() const
{
	aof_params p;
	if (!_m || !_m->ctx || aof_get_params(_m->ctx, &p)) return 0;
	return p.pyramid_levels;
}

int OpticalFlowBank::lastPushPath() const
{
	if (!_m || !_m->ctx) return 0;
	const int path = aof_bank_last_path(_m->ctx);
	return path < 0 ? 0 : path;
}

bool OpticalFlowBank::engineOk() const { return _m != NULL && !_failed; }

const char *OpticalFlowBank::lastError() const { return _err; }

const aof_outbox_entry *OpticalFlowBank::published() const
{
	return _m && _m->outbox ? reinterpret_cast<const aof_outbox_entry *>(_m->outbox + sizeof(aof_outbox_header)) : NULL;
}

const aof_exposure_command *OpticalFlowBank::exposureCommands() const { return _m && _m->camera ? _m->commands : NULL; }

int OpticalFlowBank::push(const uint8_t *frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro)
{
	if (!engineOk()) return -1;
	if (!frames || !img_time_us) return -EINVAL;
	std::memcpy(_m->stage.h, frames, _m->S * (size_t)image_width * image_height);
	return _m->tick(false, img_time_us, active, gyro);
}

int OpticalFlowBank::pushCamera(const uint8_t *sensor_frames, const uint64_t *img_time_us, const uint8_t *active,
				const aof_gyro *gyro)
{
	if (!engineOk()) return -1;
	if (!sensor_frames || !img_time_us || !_m->camera) return -EINVAL;
	std::memcpy(_m->sensor.h, sensor_frames, _m->sensor.bytes);
	return _m->tick(true, img_time_us, active, gyro);
}

// One tick on the frames push() staged in `stage`, or (sensor_frames) on those pushCamera() staged in `sensor`.  The
// body is the order of the copies and launches on the object's stream; returns the number of published entries.
int OpticalFlowBank::Impl::tick(bool sensor_frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro)
{
	std::memcpy(stage.h + off_times, img_time_us, S * sizeof(uint64_t));
	if (gyro) std::memcpy(stage.h + off_gyro, gyro, S * sizeof(aof_gyro));
	if (active) std::memcpy(stage.h + off_active, active, S);
	// What the form decides, here and nowhere else.  With the IMU form the push leaves records only (no time offset: no
	// frames) and ignores the caller's gyro: the IMU call behind it completes the records and packs the frames.
	aof_bank_params push_bp = bp;
	if (imu) push_bp.offset_timestamp_usec = 0;
	const uint64_t *d_times = reinterpret_cast<const uint64_t *>(stage.d + off_times);
	const uint8_t *d_active = active ? stage.d + off_active : NULL;
	const aof_gyro *d_gyro = gyro && !imu ? reinterpret_cast<const aof_gyro *>(stage.d + off_gyro) : NULL;
	uint8_t *push_mavlink = imu ? NULL : d_mavlink, *push_lens = imu ? NULL : d_lens;
	int rc;
	// 1. receive: the queued bytes become the samples the IMU call reads
	if (rx && (rc = receive()) != 0) return rc;
	// 2. uploads: the plain form in one copy of the whole block; sensor frames apart from the block's tail
	if (!sensor_frames) {
		if (!stage.upload(stream, 0, stage.bytes)) return fail(-EIO, "copy of the tick's frames failed");
	} else if (!sensor.upload(stream, 0, sensor.bytes) || !stage.upload(stream, off_times, stage.bytes - off_times)) {
		return fail(-EIO, "copy of the tick's sensor frames failed");
	}
	// 3. the per-stream records, if a setter changed them
	if ((rc = syncStreams()) != 0) return rc;
	// 4. the push
	rc = sensor_frames ? aof_bank_push_camera_device(ctx, &push_bp, &cam, sensor.d, d_times, d_active, d_gyro, d_bank, bank_bytes,
							 d_records, d_exposure, NULL, push_mavlink, push_lens, stream)
			   : aof_bank_push_device(ctx, &push_bp, stage.d, d_times, d_active, d_gyro, d_bank, bank_bytes, d_records,
						  push_mavlink, push_lens, stream);
	if (failed(rc)) return rc;
	// 4b. the motion field, on the limiter's own verdicts: its records land in pinned memory in front of the collect's tag
	if (field && (rc = failed(aof_bank_field_device(ctx, &push_bp, &field_params, d_bank, bank_bytes, d_records, d_field_state,
							  field_fits, field_records, stream))) != 0)
		return rc;
	// 5. the IMU call, in place on the push's records
	if (imu && (rc = takeImu()) != 0) return rc;
	// 6. the exposure control: its commands land in pinned memory in front of the collect's tag
	if (sensor_frames && (rc = failed(aof_bank_exposure_control_device(ctx, &ec, (int)S, 1, d_exposure, d_exposure_state,
									    commands, stream))) != 0)
		return rc;
	// 7. collect, and the bounded wait for it
	return collect();
}

// In front of a tick: the queued bytes to the device and the receive launch, which leaves the samples and their counts
// where takeImu()'s IMU call reads them (collect() empties the queue once the tick is through).
int OpticalFlowBank::Impl::receive()
{
	if (!bytes.upload(stream, 0, bytes.bytes)) return fail(-EIO, "copy of the tick's MAVLink bytes failed");
	return failed(aof_bank_mavlink_rx_device(ctx, &rp, bytes.d, reinterpret_cast<const uint16_t *>(bytes.d + off_rx_len), d_rx_state,
						 reinterpret_cast<aof_imu_sample *>(samples.d), samples.d + off_imu_counts, stream));
}

// In front of a tick: every per-stream table a setter has touched goes to the device if it is dirty and is bound to the
// context the first time (BankTableFlags::sync, bank_table.hpp) -- sensors, formats, binning, streams.
int OpticalFlowBank::Impl::syncStreams()
{
	for (int t = 0; t < kTables; t++) {
		const int rc = table[t].sync(
			[&]() { return table[t].upload(stream, 0, table[t].bytes) ? 0 : fail(-EIO, kTableCopyFailed[t]); },
			[&]() { return failed(bindTable(ctx, t, table[t].d, (int)S, sensor.bytes)) ? -EIO : 0; });
		if (rc) return rc;
	}
	return 0;
}

// Behind a records-only push: the queued samples to the device and the IMU call in place on the push's records.
int OpticalFlowBank::Impl::takeImu()
{
	// (with the receive path the samples and their counts are on the device already: receive() wrote them)
	if (!rx && !samples.upload(stream, 0, samples.bytes)) return fail(-EIO, "copy of the tick's IMU samples failed");
	return failed(aof_bank_imu_device(ctx, &ip, reinterpret_cast<const aof_imu_sample *>(samples.d), samples.d + off_imu_counts,
					  reinterpret_cast<const uint64_t *>(stage.d + off_times), d_records, d_imu_state, d_records,
					  d_mavlink, d_lens, stream));
}

// The collect launch behind a tick and the bounded poll of its tag; returns the number of published entries.
int OpticalFlowBank::Impl::collect()
{
	const uint64_t want = ++tag;
	const int rc = failed(aof_bank_collect_device(ctx, (int)S, 1, d_records, d_mavlink, d_lens, NULL, NULL, (uint32_t)S, 0, outbox,
						      outbox_bytes, want, NULL, stream));
	if (rc) return rc;
	// the tag is the kernel's last store: once it is here, so are the counts and the entries (and what earlier
	// launches on the stream released to the host: the exposure commands)
	const uint64_t *word = reinterpret_cast<const uint64_t *>(outbox);
	const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	while (__atomic_load_n(word, __ATOMIC_ACQUIRE) != want) {
		if (secondsSince(t0) > kDeadlineS) return fail(-ETIMEDOUT, "the tick did not finish within the deadline");
	}
	for (int t = 0; t < kTables; t++) table[t].tagSeen();   // the copies in front of the tick are through as well
	if (imu) std::memset(imuCounts(), 0, S);                      // the tick took the queued samples
	if (rx) std::memset(rxLengths(), 0, S * sizeof(uint16_t));    // and the queued bytes
	return (int)reinterpret_cast<const aof_outbox_header *>(outbox)->n_messages;
}

int OpticalFlowBank::reset(const uint8_t *mask)
{
	if (!engineOk()) return -1;
	const int rc = _m->startOver(mask, _m->imu);   // (the auto-exposure controllers keep what they hold)
	if (rc) return rc;
	return _m->waitIdle() ? 0 : -ETIMEDOUT;
}

int OpticalFlowBank::enableCamera(int camera_width, int camera_height, uint16_t exposure0, uint8_t gain0,
				  uint32_t exposure_interval_us)
{
	if (!engineOk()) return -1;
	return _m->enableSensorFrames(camera_width, camera_height, AOF_PIXEL_GREY8, exposure0, gain0, exposure_interval_us);
}

int OpticalFlowBank::enableCameraPacked(int camera_width, int camera_height, int format, uint16_t exposure0, uint8_t gain0,
					uint32_t exposure_interval_us)
{
	if (!engineOk()) return -1;
	int64_t group_row = 0;   // (as in setStreamPixelFormat(); the camera's own width is held to the format below)
	if (format < 0 || format > 255 || aof_bank_pixel_row_bytes((uint8_t)format, 4, &group_row))
		return refuse(-EINVAL, "enableCameraPacked(): no such format");
	return _m->enableSensorFrames(camera_width, camera_height, format, exposure0, gain0, exposure_interval_us);
}

// enableCamera() and enableCameraPacked(): sensor frames of camera_width x camera_height pixels of `format`.  With
// AOF_PIXEL_GREY8 nothing of the packed form is used or bound: the object runs as it always did.
int OpticalFlowBank::Impl::enableSensorFrames(int camera_width, int camera_height, int format, uint16_t exposure0, uint8_t gain0,
					      uint32_t exposure_interval_us)
{
	Impl *m = this;
	const int image_width = self->image_width, image_height = self->image_height, n_streams = self->n_streams;
	int64_t row_bytes = 0;   // a sensor row: (camera_width / G) * Bg bytes of the format's groups
	if (camera_width >= 1 && aof_bank_pixel_row_bytes((uint8_t)format, camera_width, &row_bytes))
		return self->refuse(-EINVAL, "enableCameraPacked(): the camera width is not whole pixel groups of the format");
	// a refused call leaves the object as it was: nothing of the object is written before the arguments are accepted
	if (m->camera) return self->refuse(-EINVAL, "enableCamera() was already called");
	if (!m->waitIdle()) return -ETIMEDOUT;
	aof_params p;
	if (aof_get_params(m->ctx, &p)) return fail(-EIO, aof_last_error(m->ctx));
	aof_bank_camera cam;
	std::memset(&cam, 0, sizeof(cam));
	cam.ingest.camera_width = camera_width;
	cam.ingest.camera_height = camera_height;
	cam.ingest.crop_width = image_width;
	cam.ingest.crop_height = image_height;
	cam.exposure_interval_us = exposure_interval_us;
	struct aof_bank_layout L;
	size_t staging = 0;
	if (camera_width < 1 || camera_height < 1 || aof_bank_camera_layout(&p, &m->bp, &cam, &L, &staging))
		return self->refuse(-EINVAL, "enableCamera(): the sensor frame cannot hold the image size");
	const size_t S = m->S;
	void *bank = NULL;
	int32_t mesh_nx = 0, mesh_ny = 0;
	if (aof_warp_mesh_size(&p, &mesh_nx, &mesh_ny)) return fail(-EIO, "the image size has no warp mesh");
	const size_t mesh_nodes = (size_t)mesh_nx * (size_t)mesh_ny;
	if (!m->mem.get(&bank, L.total_bytes, Allocations::kDevice) ||
	    !m->table[kWarps].alloc(m->mem, alignUp(S * mesh_nodes * sizeof(aof_warp_point), 16)) ||
	    !m->sensor.alloc(m->mem, S * (size_t)camera_height * (size_t)row_bytes) ||
	    !m->table[kSensors].alloc(m->mem, S * sizeof(aof_bank_sensor)) ||
	    !m->table[kFormats].alloc(m->mem, alignUp(S, 16)) ||
	    !m->table[kBins].alloc(m->mem, alignUp(S, 16)) ||
	    !m->mem.get((void **)&m->d_exposure, S * sizeof(aof_exposure_record), Allocations::kDevice) ||
	    !m->mem.get((void **)&m->d_exposure_state, S * sizeof(aof_exposure_state), Allocations::kDevice) ||
	    !m->mem.get((void **)&m->commands, S * sizeof(aof_exposure_command), Allocations::kOutbox))
		return fail(-ENOMEM, "device or pinned memory for the sensor frames could not be allocated");
	// the bank grows by the staging region of the composed path; the stream is idle
	m->mem.drop(m->d_bank);
	m->d_bank = bank;
	m->bank_bytes = L.total_bytes;
	m->cam = cam;
	for (size_t s = 0; s < S; s++) {
		// the centred record; another format than grey bytes: rows of row_bytes, frames of camera_height such rows, the crop
		// on a pixel group, and the stream's format beside it
		aof_bank_sensor *rec = m->sensorRecords() + s;
		if (format == AOF_PIXEL_GREY8)
			aof_bank_sensor_from_camera(&p, &cam, (int32_t)s, rec);
		else
			aof_bank_sensor_centred_binned(&p, (uint64_t)s * (uint64_t)camera_height * (uint64_t)row_bytes, (int32_t)row_bytes,
						       camera_width, camera_height, (uint8_t)format, 1, rec);
		m->table[kFormats].h[s] = (uint8_t)format;
	}
	std::memset(m->table[kBins].h, 1, m->table[kBins].bytes);
	m->mesh_nodes = mesh_nodes;
	for (size_t s = 0; s < S; s++) m->mesh((int)s)[0].x = AOF_WARP_NONE;   // (no stream is warped before its setter)
	if (format != AOF_PIXEL_GREY8) {
		m->table[kSensors].touch();
		m->table[kFormats].touch();
	}
	aof_exposure_control_default(&m->ec);
	std::memset(m->commands, 0, S * sizeof(aof_exposure_command));
	// every stream starts over, and every controller from exposure0 / gain0
	if (m->startOver(NULL, m->imu)) return -EIO;
	if (m->failed(aof_bank_exposure_reset_device(m->ctx, n_streams, NULL, exposure0, gain0, NULL, NULL, m->d_exposure_state, m->stream)))
		return -EIO;
	if (!m->waitIdle()) return -ETIMEDOUT;
	m->camera = true;
	return 0;
}

int OpticalFlowBank::enableImu(int max_samples, uint64_t offset0)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (m->imu) return refuse(-EINVAL, "enableImu() was already called");
	if (max_samples < 1 || max_samples > AOF_IMU_SLOTS_MAX) return refuse(-EINVAL, "enableImu(): max_samples outside 1..AOF_IMU_SLOTS_MAX");
	if (!m->waitIdle()) return -ETIMEDOUT;
	const size_t S = m->S;
	m->off_imu_counts = (size_t)max_samples * S * sizeof(aof_imu_sample);
	if (!m->samples.alloc(m->mem, alignUp(m->off_imu_counts + S, 256)) ||
	    !m->mem.get((void **)&m->d_imu_state, S * sizeof(aof_imu_state), Allocations::kDevice))
		return fail(-ENOMEM, "device or pinned memory for the IMU samples could not be allocated");
	std::memset(&m->ip, 0, sizeof(m->ip));
	m->ip.n_streams = n_streams;
	m->ip.n_rounds = 1;
	m->ip.max_samples = max_samples;
	m->ip.system_id = m->bp.system_id;
	m->ip.component_id = m->bp.component_id;
	m->ip.first_seq = m->bp.first_seq;
	m->imu_offset0 = offset0;
	if (m->startOver(NULL, true)) return -EIO;
	if (!m->waitIdle()) return -ETIMEDOUT;
	m->imu = true;
	return 0;
}

int OpticalFlowBank::enableField(const aof_field_params *fp)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (m->field) return refuse(-EINVAL, "enableField() was already called");
	aof_field_params mine;
	aof_field_params_default(&mine);
	if (fp) mine = *fp;
	// the fit's own checks, on host memory: one stream whose tick record says "no frame" reads nothing else
	aof_params p;
	if (aof_get_params(m->ctx, &p)) return fail(-EIO, aof_last_error(m->ctx));
	aof_block no_block;
	aof_tick_record no_frame;
	aof_bank_field_state scratch_state;
	aof_bank_field_record scratch_record;
	aof_bank_params one = m->bp;
	one.n_streams = 1;
	std::memset(&no_block, 0, sizeof(no_block));
	std::memset(&no_frame, 0, sizeof(no_frame));
	std::memset(&scratch_state, 0, sizeof(scratch_state));
	no_frame.quality = AOF_TICK_IDLE;
	if (aof_bank_field_host(&p, &one, NULL, &mine, &no_block, NULL, &no_frame, &scratch_state, NULL, &scratch_record))
		return refuse(-EINVAL, "enableField(): parameters outside their ranges, or an image size the fit does not serve");
	if (!m->waitIdle()) return -ETIMEDOUT;
	const size_t S = m->S;
	if (!m->mem.get((void **)&m->d_field_state, S * sizeof(aof_bank_field_state), Allocations::kDevice) ||
	    !m->mem.get((void **)&m->field_records, S * sizeof(aof_bank_field_record), Allocations::kOutbox) ||
	    !m->mem.get((void **)&m->field_fits, S * sizeof(aof_field), Allocations::kOutbox))
		return fail(-ENOMEM, "device or pinned memory for the motion field could not be allocated");
	std::memset(m->field_records, 0, S * sizeof(aof_bank_field_record));
	std::memset(m->field_fits, 0, S * sizeof(aof_field));
	m->field_params = mine;
	if (m->failed(aof_bank_field_reset_device(m->ctx, n_streams, NULL, m->d_field_state, m->stream))) return -EIO;
	if (!m->waitIdle()) return -ETIMEDOUT;
	m->field = true;
	return 0;
}

const aof_bank_field_record *OpticalFlowBank::fieldRecords() const { return _m && _m->field ? _m->field_records : NULL; }

const aof_field *OpticalFlowBank::fields() const { return _m && _m->field ? _m->field_fits : NULL; }

int OpticalFlowBank::pushImu(int stream, uint64_t time_usec, float xgyro, float ygyro, float zgyro)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (!m->imu || m->rx || stream < 0 || stream >= n_streams) return -EINVAL;   // (with the receive path the device counts)
	uint8_t *count = m->imuCounts() + stream;
	if (*count >= m->ip.max_samples) return -ENOBUFS;
	aof_imu_sample *slot = reinterpret_cast<aof_imu_sample *>(m->samples.h) + (size_t)*count * m->S + stream;
	slot->time_usec = time_usec;
	slot->xgyro = xgyro;
	slot->ygyro = ygyro;
	slot->zgyro = zgyro;
	slot->reserved = 0;
	*count += 1;
	return 0;
}

// Narrower than startOver() on purpose: the bank and the IMU state go on as they are.
int OpticalFlowBank::enableMavlinkRx(int max_bytes)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (!m->imu) return refuse(-EINVAL, "enableMavlinkRx() needs enableImu()");
	if (m->rx) return refuse(-EINVAL, "enableMavlinkRx() was already called");
	if (max_bytes < 16 || max_bytes > AOF_MAVLINK_RX_BYTES_MAX || max_bytes % 16)
		return refuse(-EINVAL, "enableMavlinkRx(): max_bytes outside 16..AOF_MAVLINK_RX_BYTES_MAX or no multiple of 16");
	if (!m->waitIdle()) return -ETIMEDOUT;
	const size_t S = m->S;
	m->off_rx_len = S * (size_t)max_bytes;
	if (!m->bytes.alloc(m->mem, alignUp(m->off_rx_len + S * sizeof(uint16_t), 256)) ||
	    !m->mem.get((void **)&m->d_rx_state, S * sizeof(aof_mavlink_rx_state), Allocations::kDevice))
		return fail(-ENOMEM, "device or pinned memory for the MAVLink bytes could not be allocated");
	m->rp.n_streams = n_streams;
	m->rp.n_rounds = 1;
	m->rp.max_bytes = max_bytes;
	m->rp.max_samples = m->ip.max_samples;
	if (m->failed(aof_bank_mavlink_rx_reset_device(m->ctx, n_streams, NULL, m->d_rx_state, m->stream))) return -EIO;
	if (!m->waitIdle()) return -ETIMEDOUT;
	// samples pushImu() queued are dropped: from here on the device writes the sample block
	std::memset(m->imuCounts(), 0, S);
	m->rx = true;
	return 0;
}

int OpticalFlowBank::pushMavlink(int stream, const uint8_t *bytes, int n)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (!m->rx || stream < 0 || stream >= n_streams || n < 0 || (n > 0 && !bytes)) return -EINVAL;
	uint16_t *len = m->rxLengths() + stream;
	if ((int)*len + n > m->rp.max_bytes) return -ENOBUFS;
	if (n) std::memcpy(m->bytes.h + (size_t)stream * (size_t)m->rp.max_bytes + *len, bytes, (size_t)n);
	*len = (uint16_t)(*len + n);
	return 0;
}
