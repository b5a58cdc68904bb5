// OpticalFlowBank (flow_bank.hpp): S cameras per push() through the stream bank of the C ABI
// (aof_bank_push_device) and its outbox (aof_bank_collect_device) in pinned host memory.  A push is one
// host-to-device copy of the pinned staging block (frames, times, masks, gyro), the tick, the collect
// launch, and a bounded poll of the outbox's tag: no stream synchronisation anywhere.  pushCamera() is the same
// on raw sensor frames (aof_bank_push_camera_device), with the auto-exposure controller
// (aof_bank_exposure_control_device) between the tick and the collect launch: its commands land in pinned
// memory in front of the tag.  With enableImu() the tick leaves records only and the IMU call
// (aof_bank_imu_device) behind it takes the samples pushImu() queued, completes the records in place and packs the
// frames, so that the collect launch lists only what the reference would have sent.  With enableMavlinkRx() the
// samples come from the device as well: the bytes pushMavlink() queued go over in one copy, and the receive launch
// (aof_bank_mavlink_rx_device) in front of the tick parses them into the sample block the IMU call reads.
// The setStream...() calls write a pinned shadow array of per-stream records (aof_bank_stream); the next push copies
// it to the device on the object's stream and, the first time, binds it to the context (aof_set_bank_streams).
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>

#include <hip/hip_runtime_api.h>

#include "aof.h"
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

}  // namespace

struct OpticalFlowBank::Impl {
	aof_ctx *ctx;
	aof_bank_params bp;
	hipStream_t stream;
	// one staging block, the same layout on both sides: frames, times, gyro, masks
	uint8_t *h_stage, *d_stage;
	size_t stage_bytes, off_times, off_gyro, off_active;
	void *d_bank;
	size_t bank_bytes;
	aof_tick_record *d_records;
	uint8_t *d_mavlink, *d_lens;
	uint8_t *outbox;   // pinned (aof_outbox_alloc_host): header, then n_streams entries
	size_t outbox_bytes;
	uint64_t tag;
	// the sensor-frame form (enableCamera): sensor frames staged apart from the block above
	bool camera;
	aof_bank_camera cam;
	aof_exposure_control ec;
	size_t sensor_bytes;               // all n_streams sensor frames
	uint8_t *h_sensor, *d_sensor;
	aof_exposure_record *d_exposure;
	aof_exposure_state *d_exposure_state;
	aof_exposure_command *commands;    // pinned (aof_outbox_alloc_host): [n_streams]
	// the IMU form (enableImu): samples queued by pushImu() for the next tick, [slots][n_streams] and their counts
	bool imu;
	aof_imu_params ip;
	uint64_t imu_offset0;
	uint8_t *h_imu, *d_imu;            // one block on both sides: aof_imu_sample [slots][n_streams], then u8 [n_streams]
	size_t imu_bytes, off_imu_counts;
	aof_imu_state *d_imu_state;
	// the receive path (enableMavlinkRx): bytes queued by pushMavlink() for the next tick, [n_streams][max_bytes], and
	// their lengths
	bool rx;
	aof_mavlink_rx_params rp;
	uint8_t *h_rx, *d_rx;              // one block on both sides: u8 [n_streams][max_bytes], then u16 [n_streams]
	size_t rx_bytes, off_rx_len;
	aof_mavlink_rx_state *d_rx_state;
	// the per-stream form (setStream...()): the shadow records start from the constructor's values; nothing is copied or
	// bound before the first setter
	aof_bank_stream *h_streams, *d_streams;   // pinned, device: [n_streams]
	bool streams_used, streams_dirty, streams_bound;
	bool streams_copying;              // a copy of the shadow is enqueued: it is through once collect() has seen the tick's tag
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
	std::memset(&m->bp, 0, sizeof(m->bp));
	m->bp.n_streams = streams;
	m->bp.focal_x = f_length_x;
	m->bp.focal_y = f_length_y;
	m->bp.output_rate = output_rate;
	m->bp.system_id = MAVLINK_SYSTEM_ID_DEFAULT;
	m->bp.component_id = MAVLINK_COMPONENT_ID_CAMERA;
	const size_t S = (size_t)streams, frame = (size_t)img_width * img_height;
	m->off_times = alignUp(S * frame, 256);
	m->off_gyro = alignUp(m->off_times + S * sizeof(uint64_t), 256);
	m->off_active = alignUp(m->off_gyro + S * sizeof(aof_gyro), 256);
	m->stage_bytes = alignUp(m->off_active + S, 256);
	struct aof_bank_layout L;
	struct aof_outbox_layout O;
	bool ok = aof_bank_layout(&p, &m->bp, &L) == 0 && aof_outbox_layout((uint32_t)streams, 0, &O) == 0;
	if (ok) {
		m->bank_bytes = L.total_bytes;
		m->outbox_bytes = O.total_bytes;
		ok = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) == hipSuccess &&
		     hipHostMalloc((void **)&m->h_stage, m->stage_bytes, hipHostMallocDefault) == hipSuccess &&
		     hipMalloc((void **)&m->d_stage, m->stage_bytes) == hipSuccess &&
		     hipMalloc(&m->d_bank, m->bank_bytes) == hipSuccess &&
		     hipMalloc((void **)&m->d_records, S * sizeof(aof_tick_record)) == hipSuccess &&
		     hipMalloc((void **)&m->d_mavlink, S * AOF_SEQ_FRAME_BYTES) == hipSuccess &&
		     hipMalloc((void **)&m->d_lens, S) == hipSuccess &&
		     hipHostMalloc((void **)&m->h_streams, S * sizeof(aof_bank_stream), hipHostMallocDefault) == hipSuccess &&
		     hipMalloc((void **)&m->d_streams, S * sizeof(aof_bank_stream)) == hipSuccess &&
		     aof_outbox_alloc_host(m->outbox_bytes, (void **)&m->outbox) == 0;
	}
	_m = m;
	if (!ok) {
		fail(-ENOMEM, "device or pinned memory for the bank could not be allocated");
		return;
	}
	std::memset(m->outbox, 0, m->outbox_bytes);
	for (size_t s = 0; s < S; s++) aof_bank_stream_from_params(&m->bp, &m->h_streams[s]);
	std::snprintf(_err, sizeof(_err), "ok");
	if (aof_bank_reset_device(m->ctx, &m->bp, NULL, m->d_bank, m->bank_bytes, m->stream)) {
		fail(-EIO, aof_last_error(m->ctx));
		return;
	}
	waitIdle();
}

OpticalFlowBank::~OpticalFlowBank()
{
	if (!_m) return;
	Impl *m = _m;
	// a bounded wait, as everywhere: memory a kernel may still write is leaked, not freed
	const bool drained = !m->stream || waitIdle();
	if (drained) {
		if (m->d_rx_state) (void)hipFree(m->d_rx_state);
		if (m->d_rx) (void)hipFree(m->d_rx);
		if (m->h_rx) (void)hipHostFree(m->h_rx);
		if (m->d_imu_state) (void)hipFree(m->d_imu_state);
		if (m->d_imu) (void)hipFree(m->d_imu);
		if (m->h_imu) (void)hipHostFree(m->h_imu);
		if (m->commands) aof_outbox_free_host(m->commands);
		if (m->d_exposure_state) (void)hipFree(m->d_exposure_state);
		if (m->d_exposure) (void)hipFree(m->d_exposure);
		if (m->d_sensor) (void)hipFree(m->d_sensor);
		if (m->h_sensor) (void)hipHostFree(m->h_sensor);
		if (m->outbox) aof_outbox_free_host(m->outbox);
		if (m->d_streams) (void)hipFree(m->d_streams);
		if (m->h_streams) (void)hipHostFree(m->h_streams);
		if (m->d_lens) (void)hipFree(m->d_lens);
		if (m->d_mavlink) (void)hipFree(m->d_mavlink);
		if (m->d_records) (void)hipFree(m->d_records);
		if (m->d_bank) (void)hipFree(m->d_bank);
		if (m->d_stage) (void)hipFree(m->d_stage);
		if (m->h_stage) (void)hipHostFree(m->h_stage);
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
bool OpticalFlowBank::waitIdle()
{
	const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	for (;;) {
		const hipError_t e = hipStreamQuery(_m->stream);
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

void OpticalFlowBank::setTimestampOffset(uint64_t offset_usec)
{
	if (!_m) return;
	_m->bp.offset_timestamp_usec = offset_usec;
	if (!_m->h_streams) return;
	for (int s = 0; s < n_streams; s++) _m->h_streams[s].offset_timestamp_usec = offset_usec;
	_m->streams_dirty = true;
}

// The shadow record of stream s for a setter, or NULL (bad index, no engine); the next push copies the array.
aof_bank_stream *OpticalFlowBank::streamRecord(int s)
{
	if (!_m || !_m->h_streams || s < 0 || s >= n_streams) return NULL;
	_m->streams_used = true;
	_m->streams_dirty = true;
	return &_m->h_streams[s];
}

int OpticalFlowBank::setStreamFocalLength(int s, float f_length_x, float f_length_y)
{
	if (!(f_length_x > 0.0f) || !(f_length_y > 0.0f)) return -EINVAL;
	aof_bank_stream *r = streamRecord(s);
	if (!r) return -EINVAL;
	r->focal_x = f_length_x;
	r->focal_y = f_length_y;
	return 0;
}

int OpticalFlowBank::setStreamOutputRate(int s, int output_rate)
{
	aof_bank_stream *r = streamRecord(s);
	if (!r) return -EINVAL;
	r->output_rate = output_rate;
	return 0;
}

int OpticalFlowBank::setStreamIdentity(int s, uint8_t system_id, uint8_t component_id, uint8_t first_seq)
{
	aof_bank_stream *r = streamRecord(s);
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
	aof_bank_stream *r = streamRecord(s);
	if (!r) return -EINVAL;
	r->offset_timestamp_usec = offset_usec;
	return 0;
}

// In front of a tick: the shadow records to the device if a setter changed them, and bound to the context the first
// time.  Without a setter nothing happens: the tick runs on the scalars, as it always did.  The shadow counts as copied
// only once collect() has waited for the tick: a setter behind a push that failed in between writes an array that is
// still marked dirty, and the object has failed for good by then.
int OpticalFlowBank::syncStreams()
{
	Impl *m = _m;
	if (!m->streams_used) return 0;
	if (m->streams_dirty) {
		if (hipMemcpyAsync(m->d_streams, m->h_streams, (size_t)n_streams * sizeof(aof_bank_stream), hipMemcpyHostToDevice,
				   m->stream) != hipSuccess)
			return fail(-EIO, "copy of the per-stream records failed");
		// (still dirty: only collect(), which waits for the tick, knows that the copy has read the shadow; a push that
		// fails behind this point copies again)
		m->streams_copying = true;
	}
	if (!m->streams_bound) {
		if (aof_set_bank_streams(m->ctx, m->d_streams, n_streams)) return fail(-EIO, aof_last_error(m->ctx));
		m->streams_bound = true;
	}
	return 0;
}

int OpticalFlowBank::getPyramidLevels() const
{
	aof_params p;
	if (!_m || !_m->ctx || aof_get_params(_m->ctx, &p)) return 0;
	return p.pyramid_levels;
}

bool OpticalFlowBank::engineOk() const { return _m != NULL && !_failed; }

const char *OpticalFlowBank::lastError() const { return _err; }

const aof_outbox_entry *OpticalFlowBank::published() const
{
	return _m && _m->outbox ? reinterpret_cast<const aof_outbox_entry *>(_m->outbox + sizeof(aof_outbox_header)) : NULL;
}

int OpticalFlowBank::push(const uint8_t *frames, const uint64_t *img_time_us, const uint8_t *active, const aof_gyro *gyro)
{
	if (!engineOk()) return -1;
	if (!frames || !img_time_us) return -EINVAL;
	Impl *m = _m;
	const size_t S = (size_t)n_streams, frame = (size_t)image_width * image_height;
	std::memcpy(m->h_stage, frames, S * frame);
	std::memcpy(m->h_stage + m->off_times, img_time_us, S * sizeof(uint64_t));
	if (gyro) std::memcpy(m->h_stage + m->off_gyro, gyro, S * sizeof(aof_gyro));
	if (active) std::memcpy(m->h_stage + m->off_active, active, S);
	if (m->rx) {
		const int rrc = receive();
		if (rrc) return rrc;
	}
	if (hipMemcpyAsync(m->d_stage, m->h_stage, m->stage_bytes, hipMemcpyHostToDevice, m->stream) != hipSuccess)
		return fail(-EIO, "copy of the tick's frames failed");
	int rc = syncStreams();
	if (rc) return rc;
	// with the IMU form the tick leaves records only: the IMU call behind it completes them and packs the frames
	aof_bank_params bp = m->bp;
	if (m->imu) bp.offset_timestamp_usec = 0;
	rc = aof_bank_push_device(m->ctx, &bp, m->d_stage, reinterpret_cast<const uint64_t *>(m->d_stage + m->off_times),
				      active ? m->d_stage + m->off_active : NULL,
				      gyro && !m->imu ? reinterpret_cast<const aof_gyro *>(m->d_stage + m->off_gyro) : NULL, m->d_bank,
				      m->bank_bytes, m->d_records, m->imu ? NULL : m->d_mavlink, m->imu ? NULL : m->d_lens, m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	if (m->imu && (rc = takeImu()) != 0) return rc;
	return collect();
}

// The collect launch behind a tick and the bounded poll of its tag; returns the number of published entries.
int OpticalFlowBank::collect()
{
	Impl *m = _m;
	const uint64_t tag = ++m->tag;
	const int rc = aof_bank_collect_device(m->ctx, n_streams, 1, m->d_records, m->d_mavlink, m->d_lens, NULL, NULL,
					       (uint32_t)n_streams, 0, m->outbox, m->outbox_bytes, tag, NULL, m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	// the tag is the kernel's last store: once it is here, so are the counts and the entries (and what earlier
	// launches on the stream released to the host: the exposure commands)
	const uint64_t *word = reinterpret_cast<const uint64_t *>(m->outbox);
	const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	while (__atomic_load_n(word, __ATOMIC_ACQUIRE) != tag) {
		if (secondsSince(t0) > kDeadlineS) return fail(-ETIMEDOUT, "the tick did not finish within the deadline");
	}
	if (m->streams_copying) {   // the copy of the per-stream records in front of the tick is through as well
		m->streams_copying = false;
		m->streams_dirty = false;
	}
	if (m->imu) std::memset(m->h_imu + m->off_imu_counts, 0, (size_t)n_streams);   // the tick took the queued samples
	if (m->rx) std::memset(m->h_rx + m->off_rx_len, 0, (size_t)n_streams * sizeof(uint16_t));   // and the queued bytes
	return (int)reinterpret_cast<const aof_outbox_header *>(m->outbox)->n_messages;
}

int OpticalFlowBank::enableCamera(int camera_width, int camera_height, uint16_t exposure0, uint8_t gain0,
				  uint32_t exposure_interval_us)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	// a wrong argument is refused and leaves the object as it was
	if (m->camera) return refuse(-EINVAL, "enableCamera() was already called");
	if (!waitIdle()) return -ETIMEDOUT;
	aof_params p;
	if (aof_get_params(m->ctx, &p)) return fail(-EIO, aof_last_error(m->ctx));
	std::memset(&m->cam, 0, sizeof(m->cam));
	m->cam.ingest.camera_width = camera_width;
	m->cam.ingest.camera_height = camera_height;
	m->cam.ingest.crop_width = image_width;
	m->cam.ingest.crop_height = image_height;
	m->cam.exposure_interval_us = exposure_interval_us;
	struct aof_bank_layout L;
	size_t staging = 0;
	if (camera_width < 1 || camera_height < 1 || aof_bank_camera_layout(&p, &m->bp, &m->cam, &L, &staging))
		return refuse(-EINVAL, "enableCamera(): the sensor frame cannot hold the image size");
	const size_t S = (size_t)n_streams;
	m->sensor_bytes = S * (size_t)camera_width * (size_t)camera_height;
	aof_exposure_control_default(&m->ec);
	void *bank = NULL;
	const bool ok = hipMalloc(&bank, L.total_bytes) == hipSuccess &&
			hipHostMalloc((void **)&m->h_sensor, m->sensor_bytes, hipHostMallocDefault) == hipSuccess &&
			hipMalloc((void **)&m->d_sensor, m->sensor_bytes) == hipSuccess &&
			hipMalloc((void **)&m->d_exposure, S * sizeof(aof_exposure_record)) == hipSuccess &&
			hipMalloc((void **)&m->d_exposure_state, S * sizeof(aof_exposure_state)) == hipSuccess &&
			aof_outbox_alloc_host(S * sizeof(aof_exposure_command), (void **)&m->commands) == 0;
	if (bank) {   // the bank grows by the staging region of the composed path; the stream is idle
		(void)hipFree(m->d_bank);
		m->d_bank = bank;
		m->bank_bytes = L.total_bytes;
	}
	if (!ok) return fail(-ENOMEM, "device or pinned memory for the sensor frames could not be allocated");
	std::memset(m->commands, 0, S * sizeof(aof_exposure_command));
	if (aof_bank_reset_device(m->ctx, &m->bp, NULL, m->d_bank, m->bank_bytes, m->stream) ||
	    aof_bank_exposure_reset_device(m->ctx, n_streams, NULL, exposure0, gain0, NULL, NULL, m->d_exposure_state, m->stream))
		return fail(-EIO, aof_last_error(m->ctx));
	if (m->imu) {   // every stream starts over: its IMU state and the samples queued for it as well
		if (aof_bank_imu_reset_device(m->ctx, n_streams, NULL, m->imu_offset0, m->d_imu_state, m->stream))
			return fail(-EIO, aof_last_error(m->ctx));
		std::memset(m->h_imu + m->off_imu_counts, 0, (size_t)n_streams);
	}
	if (m->rx) {    // and its receive state and queued bytes
		if (aof_bank_mavlink_rx_reset_device(m->ctx, n_streams, NULL, m->d_rx_state, m->stream))
			return fail(-EIO, aof_last_error(m->ctx));
		std::memset(m->h_rx + m->off_rx_len, 0, (size_t)n_streams * sizeof(uint16_t));
	}
	if (!waitIdle()) return -ETIMEDOUT;
	m->camera = true;
	return 0;
}

const aof_exposure_command *OpticalFlowBank::exposureCommands() const { return _m && _m->camera ? _m->commands : NULL; }

int OpticalFlowBank::pushCamera(const uint8_t *sensor_frames, const uint64_t *img_time_us, const uint8_t *active,
				const aof_gyro *gyro)
{
	if (!engineOk()) return -1;
	if (!sensor_frames || !img_time_us || !_m->camera) return -EINVAL;
	Impl *m = _m;
	const size_t S = (size_t)n_streams;
	std::memcpy(m->h_sensor, sensor_frames, m->sensor_bytes);
	std::memcpy(m->h_stage + m->off_times, img_time_us, S * sizeof(uint64_t));
	if (gyro) std::memcpy(m->h_stage + m->off_gyro, gyro, S * sizeof(aof_gyro));
	if (active) std::memcpy(m->h_stage + m->off_active, active, S);
	if (m->rx) {
		const int rrc = receive();
		if (rrc) return rrc;
	}
	if (hipMemcpyAsync(m->d_sensor, m->h_sensor, m->sensor_bytes, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
	    hipMemcpyAsync(m->d_stage + m->off_times, m->h_stage + m->off_times, m->stage_bytes - m->off_times,
			   hipMemcpyHostToDevice, m->stream) != hipSuccess)
		return fail(-EIO, "copy of the tick's sensor frames failed");
	int rc = syncStreams();
	if (rc) return rc;
	aof_bank_params bp = m->bp;
	if (m->imu) bp.offset_timestamp_usec = 0;   // (records only, as in push())
	rc = aof_bank_push_camera_device(m->ctx, &bp, &m->cam, m->d_sensor,
					     reinterpret_cast<const uint64_t *>(m->d_stage + m->off_times),
					     active ? m->d_stage + m->off_active : NULL,
					     gyro && !m->imu ? reinterpret_cast<const aof_gyro *>(m->d_stage + m->off_gyro) : NULL, m->d_bank,
					     m->bank_bytes, m->d_records, m->d_exposure, NULL, m->imu ? NULL : m->d_mavlink,
					     m->imu ? NULL : m->d_lens, m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	if (m->imu && (rc = takeImu()) != 0) return rc;
	rc = aof_bank_exposure_control_device(m->ctx, &m->ec, n_streams, 1, m->d_exposure, m->d_exposure_state, m->commands,
					      m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	return collect();
}

int OpticalFlowBank::reset(const uint8_t *mask)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (mask) {
		std::memcpy(m->h_stage + m->off_active, mask, (size_t)n_streams);
		if (hipMemcpyAsync(m->d_stage + m->off_active, m->h_stage + m->off_active, (size_t)n_streams, hipMemcpyHostToDevice,
				   m->stream) != hipSuccess)
			return fail(-EIO, "copy of the reset mask failed");
	}
	int rc = aof_bank_reset_device(m->ctx, &m->bp, mask ? m->d_stage + m->off_active : NULL, m->d_bank, m->bank_bytes,
				       m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	if (m->imu) {
		rc = aof_bank_imu_reset_device(m->ctx, n_streams, mask ? m->d_stage + m->off_active : NULL, m->imu_offset0,
					       m->d_imu_state, m->stream);
		if (rc) return fail(rc, aof_last_error(m->ctx));
		// samples queued for a stream that starts over belong to its past: they are dropped with it
		uint8_t *counts = m->h_imu + m->off_imu_counts;
		for (int s = 0; s < n_streams; s++)
			if (!mask || mask[s]) counts[s] = 0;
	}
	if (m->rx) {   // likewise a frame half received and the bytes queued
		rc = aof_bank_mavlink_rx_reset_device(m->ctx, n_streams, mask ? m->d_stage + m->off_active : NULL, m->d_rx_state,
						      m->stream);
		if (rc) return fail(rc, aof_last_error(m->ctx));
		uint16_t *lens = reinterpret_cast<uint16_t *>(m->h_rx + m->off_rx_len);
		for (int s = 0; s < n_streams; s++)
			if (!mask || mask[s]) lens[s] = 0;
	}
	return waitIdle() ? 0 : -ETIMEDOUT;
}

int OpticalFlowBank::enableImu(int max_samples, uint64_t offset0)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (m->imu) return refuse(-EINVAL, "enableImu() was already called");
	if (max_samples < 1 || max_samples > AOF_IMU_SLOTS_MAX) return refuse(-EINVAL, "enableImu(): max_samples outside 1..AOF_IMU_SLOTS_MAX");
	if (!waitIdle()) return -ETIMEDOUT;
	const size_t S = (size_t)n_streams;
	m->off_imu_counts = (size_t)max_samples * S * sizeof(aof_imu_sample);
	m->imu_bytes = alignUp(m->off_imu_counts + S, 256);
	const bool ok = hipHostMalloc((void **)&m->h_imu, m->imu_bytes, hipHostMallocDefault) == hipSuccess &&
			hipMalloc((void **)&m->d_imu, m->imu_bytes) == hipSuccess &&
			hipMalloc((void **)&m->d_imu_state, S * sizeof(aof_imu_state)) == hipSuccess;
	if (!ok) return fail(-ENOMEM, "device or pinned memory for the IMU samples could not be allocated");
	std::memset(m->h_imu, 0, m->imu_bytes);
	std::memset(&m->ip, 0, sizeof(m->ip));
	m->ip.n_streams = n_streams;
	m->ip.n_rounds = 1;
	m->ip.max_samples = max_samples;
	m->ip.system_id = m->bp.system_id;
	m->ip.component_id = m->bp.component_id;
	m->ip.first_seq = m->bp.first_seq;
	m->imu_offset0 = offset0;
	if (aof_bank_reset_device(m->ctx, &m->bp, NULL, m->d_bank, m->bank_bytes, m->stream) ||
	    aof_bank_imu_reset_device(m->ctx, n_streams, NULL, offset0, m->d_imu_state, m->stream))
		return fail(-EIO, aof_last_error(m->ctx));
	if (!waitIdle()) return -ETIMEDOUT;
	m->imu = true;
	return 0;
}

int OpticalFlowBank::pushImu(int stream, uint64_t time_usec, float xgyro, float ygyro, float zgyro)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (!m->imu || m->rx || stream < 0 || stream >= n_streams) return -EINVAL;   // (with the receive path the device counts)
	uint8_t *count = m->h_imu + m->off_imu_counts + stream;
	if (*count >= m->ip.max_samples) return -ENOBUFS;
	aof_imu_sample *slot = reinterpret_cast<aof_imu_sample *>(m->h_imu) + (size_t)*count * (size_t)n_streams + stream;
	slot->time_usec = time_usec;
	slot->xgyro = xgyro;
	slot->ygyro = ygyro;
	slot->zgyro = zgyro;
	slot->reserved = 0;
	*count += 1;
	return 0;
}

// Behind a records-only tick: the queued samples to the device, the IMU call in place on the tick's records, and the
// queue is empty again (collect() waits for the tick, so the pinned block is free when push() returns).
int OpticalFlowBank::takeImu()
{
	Impl *m = _m;
	// (with the receive path the samples and their counts are on the device already: receive() wrote them)
	if (!m->rx && hipMemcpyAsync(m->d_imu, m->h_imu, m->imu_bytes, hipMemcpyHostToDevice, m->stream) != hipSuccess)
		return fail(-EIO, "copy of the tick's IMU samples failed");
	const int rc = aof_bank_imu_device(m->ctx, &m->ip, reinterpret_cast<const aof_imu_sample *>(m->d_imu), m->d_imu + m->off_imu_counts,
					   reinterpret_cast<const uint64_t *>(m->d_stage + m->off_times), m->d_records, m->d_imu_state,
					   m->d_records, m->d_mavlink, m->d_lens, m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	return 0;
}

int OpticalFlowBank::enableMavlinkRx(int max_bytes)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (!m->imu) return refuse(-EINVAL, "enableMavlinkRx() needs enableImu()");
	if (m->rx) return refuse(-EINVAL, "enableMavlinkRx() was already called");
	if (max_bytes < 16 || max_bytes > AOF_MAVLINK_RX_BYTES_MAX || max_bytes % 16)
		return refuse(-EINVAL, "enableMavlinkRx(): max_bytes outside 16..AOF_MAVLINK_RX_BYTES_MAX or no multiple of 16");
	if (!waitIdle()) return -ETIMEDOUT;
	const size_t S = (size_t)n_streams;
	m->off_rx_len = S * (size_t)max_bytes;
	m->rx_bytes = alignUp(m->off_rx_len + S * sizeof(uint16_t), 256);
	const bool ok = hipHostMalloc((void **)&m->h_rx, m->rx_bytes, hipHostMallocDefault) == hipSuccess &&
			hipMalloc((void **)&m->d_rx, m->rx_bytes) == hipSuccess &&
			hipMalloc((void **)&m->d_rx_state, S * sizeof(aof_mavlink_rx_state)) == hipSuccess;
	if (!ok) return fail(-ENOMEM, "device or pinned memory for the MAVLink bytes could not be allocated");
	std::memset(m->h_rx, 0, m->rx_bytes);
	m->rp.n_streams = n_streams;
	m->rp.n_rounds = 1;
	m->rp.max_bytes = max_bytes;
	m->rp.max_samples = m->ip.max_samples;
	if (aof_bank_mavlink_rx_reset_device(m->ctx, n_streams, NULL, m->d_rx_state, m->stream))
		return fail(-EIO, aof_last_error(m->ctx));
	if (!waitIdle()) return -ETIMEDOUT;
	// samples pushImu() queued are dropped: from here on the device writes the sample block
	std::memset(m->h_imu + m->off_imu_counts, 0, S);
	m->rx = true;
	return 0;
}

int OpticalFlowBank::pushMavlink(int stream, const uint8_t *bytes, int n)
{
	if (!engineOk()) return -1;
	Impl *m = _m;
	if (!m->rx || stream < 0 || stream >= n_streams || n < 0 || (n > 0 && !bytes)) return -EINVAL;
	uint16_t *len = reinterpret_cast<uint16_t *>(m->h_rx + m->off_rx_len) + stream;
	if ((int)*len + n > m->rp.max_bytes) return -ENOBUFS;
	if (n) std::memcpy(m->h_rx + (size_t)stream * (size_t)m->rp.max_bytes + *len, bytes, (size_t)n);
	*len = (uint16_t)(*len + n);
	return 0;
}

// In front of a tick: the queued bytes to the device and the receive launch, which leaves the samples and their counts
// where takeImu()'s IMU call reads them (collect() empties the queue once the tick is through).
int OpticalFlowBank::receive()
{
	Impl *m = _m;
	if (hipMemcpyAsync(m->d_rx, m->h_rx, m->rx_bytes, hipMemcpyHostToDevice, m->stream) != hipSuccess)
		return fail(-EIO, "copy of the tick's MAVLink bytes failed");
	const int rc = aof_bank_mavlink_rx_device(m->ctx, &m->rp, m->d_rx, reinterpret_cast<const uint16_t *>(m->d_rx + m->off_rx_len),
						  m->d_rx_state, reinterpret_cast<aof_imu_sample *>(m->d_imu), m->d_imu + m->off_imu_counts,
						  m->stream);
	if (rc) return fail(rc, aof_last_error(m->ctx));
	return 0;
}
