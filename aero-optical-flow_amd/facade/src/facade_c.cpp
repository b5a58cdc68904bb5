// Plain-C handles on the facade classes, so that non-C++ harnesses (the Python
// tests via ctypes) drive the real C++ classes rather than a re-implementation.
// Nothing throws across the C boundary: the classes are made with new (std::nothrow) -- a null handle
// tells the caller, as /root/reference/src/mainloop.cpp:425-428 checks its own `new` -- and the one array
// a delegate needs likewise.
#include <new>

#include "flow_bank.hpp"
#include "flow_opencv.hpp"
#include "flow_px4.hpp"
#include "optical_flow_rad.hpp"

extern "C" {

void *aof_facade_px4_create(float fx, float fy, int output_rate, int w, int h, int search,
			    int feature_threshold, int value_threshold)
{
	return new (std::nothrow) OpticalFlowPX4(fx, fy, output_rate, w, h, search, feature_threshold,
						 value_threshold);
}

void *aof_facade_opencv_create(float fx, float fy, int output_rate, int w, int h)
{
	// exactly the five arguments /root/reference/src/mainloop.cpp:423-424 passes
	return new (std::nothrow) OpticalFlowOpenCV(fx, fy, output_rate, w, h);
}

void aof_facade_destroy(void *flow) { delete static_cast<OpticalFlow *>(flow); }

int aof_facade_calc_flow(void *flow, uint8_t *img, uint32_t t_us, int *dt_us, float *flow_x,
			 float *flow_y)
{
	return static_cast<OpticalFlow *>(flow)->calcFlow(img, t_us, *dt_us, *flow_x, *flow_y);
}

int aof_facade_px4_track_features(void *flow, const uint8_t *prev, const uint8_t *cur, float *out6, int capacity)
{
	// out6: capacity rows of {prev_x, prev_y, cur_x, cur_y, sad, accepted}
	OpticalFlowPX4 *px4 = static_cast<OpticalFlowPX4 *>(flow);
	TrackedFeature *tmp = new (std::nothrow) TrackedFeature[capacity > 0 ? capacity : 1];
	if (!tmp) return -1;
	int n = px4->trackFeatures(prev, cur, tmp, capacity);
	for (int k = 0; k < n && k < capacity; k++) {
		out6[6 * k + 0] = tmp[k].prev_x; out6[6 * k + 1] = tmp[k].prev_y;
		out6[6 * k + 2] = tmp[k].cur_x;  out6[6 * k + 3] = tmp[k].cur_y;
		out6[6 * k + 4] = (float)tmp[k].sad; out6[6 * k + 5] = tmp[k].accepted ? 1.0f : 0.0f;
	}
	delete[] tmp;
	return n;
}

int aof_facade_pack_optical_flow_rad(uint64_t offset_ts, uint64_t img_time_us, int dt_us, float fx, float fy,
				     double gyro_x, double gyro_y, double gyro_z, int quality, uint8_t seq,
				     uint8_t *out56)
{
	OpticalFlowRad m;
	fillOpticalFlowRad(m, offset_ts, img_time_us, dt_us, fx, fy, gyro_x, gyro_y, gyro_z, quality);
	return (int)packOpticalFlowRad(m, seq, MAVLINK_SYSTEM_ID_DEFAULT, MAVLINK_COMPONENT_ID_CAMERA, out56);
}

unsigned aof_facade_mavlink_crc(const uint8_t *data, int len) { return mavlinkCrcAccumulate(data, (size_t)len, 0xFFFF); }

int aof_facade_set_search_pyramid(void *flow, int levels, int mean_subtract)
{
	return static_cast<OpticalFlow *>(flow)->setSearchPyramid(levels, mean_subtract != 0) ? 1 : 0;
}
int aof_facade_pyramid_levels(void *flow) { return static_cast<OpticalFlow *>(flow)->getPyramidLevels(); }
int aof_facade_set_resident(void *flow, int on) { return static_cast<OpticalFlow *>(flow)->setResidentKernel(on != 0) ? 1 : 0; }

int aof_facade_image_width(void *flow) { return static_cast<OpticalFlow *>(flow)->getImageWidth(); }
int aof_facade_image_height(void *flow) { return static_cast<OpticalFlow *>(flow)->getImageHeight(); }
const char *aof_facade_last_error(void *flow) { return static_cast<OpticalFlow *>(flow)->lastError(); }
int aof_facade_default_output_rate(void) { return DEFAULT_OUTPUT_RATE; }

// ---- OpticalFlowBank (flow_bank.hpp) ----
void *aof_facade_bank_create(float fx, float fy, int output_rate, int w, int h, int n_streams)
{
	return new (std::nothrow) OpticalFlowBank(fx, fy, output_rate, w, h, n_streams);
}
void aof_facade_bank_destroy(void *bank) { delete static_cast<OpticalFlowBank *>(bank); }
void aof_facade_bank_set_timestamp_offset(void *bank, uint64_t offset_usec)
{
	static_cast<OpticalFlowBank *>(bank)->setTimestampOffset(offset_usec);
}
int aof_facade_bank_set_stream_focal_length(void *bank, int stream, float fx, float fy)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamFocalLength(stream, fx, fy);
}
int aof_facade_bank_set_stream_output_rate(void *bank, int stream, int output_rate)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamOutputRate(stream, output_rate);
}
int aof_facade_bank_set_stream_identity(void *bank, int stream, int system_id, int component_id, int first_seq)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamIdentity(stream, (uint8_t)system_id, (uint8_t)component_id, (uint8_t)first_seq);
}
int aof_facade_bank_set_stream_timestamp_offset(void *bank, int stream, uint64_t offset_usec)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamTimestampOffset(stream, offset_usec);
}
int aof_facade_bank_set_stream_sensor(void *bank, int stream, uint64_t offset, int pitch, int width, int height, int x0, int y0)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamSensor(stream, offset, pitch, width, height, x0, y0);
}
int aof_facade_bank_set_stream_pixel_format(void *bank, int stream, int format)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamPixelFormat(stream, format);
}
int aof_facade_bank_set_stream_binning(void *bank, int stream, int bin)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamBinning(stream, bin);
}
int aof_facade_bank_set_stream_warp(void *bank, int stream, const void *mesh)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamWarp(stream, static_cast<const aof_warp_point *>(mesh));
}
int aof_facade_bank_set_stream_lens(void *bank, int stream, double fx, double fy, double cx, double cy, double k1, double k2, double p1,
				    double p2, double k3)
{
	return static_cast<OpticalFlowBank *>(bank)->setStreamLens(stream, fx, fy, cx, cy, k1, k2, p1, p2, k3);
}
int aof_facade_bank_enable_camera_packed(void *bank, int camera_width, int camera_height, int format, int exposure0, int gain0,
					 uint32_t exposure_interval_us)
{
	return static_cast<OpticalFlowBank *>(bank)->enableCameraPacked(camera_width, camera_height, format, (uint16_t)exposure0,
									 (uint8_t)gain0, exposure_interval_us);
}
int aof_facade_bank_push(void *bank, const uint8_t *frames, const uint64_t *img_time_us, const uint8_t *active,
			 const aof_gyro *gyro)
{
	return static_cast<OpticalFlowBank *>(bank)->push(frames, img_time_us, active, gyro);
}
int aof_facade_bank_enable_camera(void *bank, int camera_width, int camera_height, int exposure0, int gain0,
				  uint32_t exposure_interval_us)
{
	return static_cast<OpticalFlowBank *>(bank)->enableCamera(camera_width, camera_height, (uint16_t)exposure0, (uint8_t)gain0,
								   exposure_interval_us);
}
int aof_facade_bank_push_camera(void *bank, const uint8_t *sensor_frames, const uint64_t *img_time_us, const uint8_t *active,
				const aof_gyro *gyro)
{
	return static_cast<OpticalFlowBank *>(bank)->pushCamera(sensor_frames, img_time_us, active, gyro);
}
int aof_facade_bank_enable_imu(void *bank, int max_samples, uint64_t offset0)
{
	return static_cast<OpticalFlowBank *>(bank)->enableImu(max_samples, offset0);
}
int aof_facade_bank_push_imu(void *bank, int stream, uint64_t time_usec, float xgyro, float ygyro, float zgyro)
{
	return static_cast<OpticalFlowBank *>(bank)->pushImu(stream, time_usec, xgyro, ygyro, zgyro);
}
int aof_facade_bank_enable_mavlink_rx(void *bank, int max_bytes)
{
	return static_cast<OpticalFlowBank *>(bank)->enableMavlinkRx(max_bytes);
}
int aof_facade_bank_push_mavlink(void *bank, int stream, const uint8_t *bytes, int n)
{
	return static_cast<OpticalFlowBank *>(bank)->pushMavlink(stream, bytes, n);
}
int aof_facade_bank_enable_field(void *bank, const void *field_params)
{
	return static_cast<OpticalFlowBank *>(bank)->enableField(static_cast<const aof_field_params *>(field_params));
}
const void *aof_facade_bank_field_records(void *bank) { return static_cast<OpticalFlowBank *>(bank)->fieldRecords(); }
const void *aof_facade_bank_fields(void *bank) { return static_cast<OpticalFlowBank *>(bank)->fields(); }
const void *aof_facade_bank_exposure_commands(void *bank) { return static_cast<OpticalFlowBank *>(bank)->exposureCommands(); }
const void *aof_facade_bank_published(void *bank) { return static_cast<OpticalFlowBank *>(bank)->published(); }
int aof_facade_bank_reset(void *bank, const uint8_t *mask) { return static_cast<OpticalFlowBank *>(bank)->reset(mask); }
int aof_facade_bank_pyramid_levels(void *bank) { return static_cast<OpticalFlowBank *>(bank)->getPyramidLevels(); }
int aof_facade_bank_last_push_path(void *bank) { return static_cast<OpticalFlowBank *>(bank)->lastPushPath(); }
int aof_facade_bank_ok(void *bank) { return static_cast<OpticalFlowBank *>(bank)->engineOk() ? 1 : 0; }
const char *aof_facade_bank_last_error(void *bank) { return static_cast<OpticalFlowBank *>(bank)->lastError(); }

}  // extern "C"
