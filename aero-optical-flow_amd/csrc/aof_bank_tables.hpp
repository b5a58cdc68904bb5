// The stream bank's bound per-stream tables (include/aof.h: aof_set_bank_streams, aof_set_bank_sensors,
// aof_set_bank_pixel_formats, aof_set_bank_binning): each a caller-owned device array for S streams, bound to the context
// and read by the kernels when they run.  One record of what is bound (BankTables, a member of aof_ctx), and the rules
// over it as plain functions that know no context: what a binding call accepts, which tables a push or an IMU call of
// n_streams uses and why it is refused, and the kernels' sensor arguments of one round.  Host only: a CPU program can
// call all of it (tests/native/host_selftest.cpp).  A further per-stream array is one more BankTable and one more line
// in each rule.
#pragma once

#include <cstdint>

#include "aof.h"
#include "aof_bank_args.hpp"     // BankSensors
#include "aof_host.hpp"          // aligned
#include "aof_ingest_args.hpp"   // IngestSensors

namespace aof {

enum BankTable { kBankStreams, kBankSensors, kBankFormats, kBankBins, kBankTableCount };

struct BankTables {
    struct Bound {
        const void *array;     // device memory of the caller's, or nullptr: nothing bound
        int32_t n_streams;     // how many streams it is for (0 with nothing bound)
    } table[kBankTableCount];
    uint64_t camera_bytes;     // with sensor records: bytes the caller guarantees readable from the d_camera of its pushes
};

inline bool operator==(const BankTables &a, const BankTables &b)
{
    for (int t = 0; t < kBankTableCount; t++)
        if (a.table[t].array != b.table[t].array || a.table[t].n_streams != b.table[t].n_streams) return false;
    return a.camera_bytes == b.camera_bytes;
}

// The binding calls: nullptr, or why the call is refused -- the binding is then as it was.  A null array unbinds.
// camera_bytes: of the sensor records, not looked at otherwise.
inline const char *bank_tables_bind(BankTables *b, BankTable which, const void *array, int32_t n_streams, uint64_t camera_bytes = 0)
{
    static const struct { const char *no_streams, *misaligned; } kRefusal[kBankTableCount] = {
        {"bank streams: an array needs n_streams >= 1", "bank streams: the array must be 16-byte aligned"},
        {"bank sensors: an array needs n_streams >= 1", "bank sensors: the array must be 16-byte aligned"},
        {"bank pixel formats: an array needs n_streams >= 1", nullptr},   // (bytes: any alignment)
        {"bank binning: an array needs n_streams >= 1", nullptr},
    };
    if (array && n_streams < 1) return kRefusal[which].no_streams;
    if (kRefusal[which].misaligned && !aligned(array, 16)) return kRefusal[which].misaligned;
    if (which == kBankSensors) {
        if (array && camera_bytes == 0) return "bank sensors: an array needs camera_bytes > 0";
        b->camera_bytes = array ? camera_bytes : 0;
    }
    b->table[which].array = array;
    b->table[which].n_streams = array ? n_streams : 0;
    return nullptr;
}

// The tables one call uses: what is bound, for the call's stream count.
struct BankTablesUsed {
    const aof_bank_stream *streams;
    const aof_bank_sensor *sensors;
    uint64_t camera_bytes;
    const uint8_t *formats, *bins;
};

// A bound array is for one stream count: the kernels index it by the stream.
inline bool bank_table_differs(const BankTables &b, BankTable which, int32_t n_streams)
{
    return b.table[which].array && b.table[which].n_streams != n_streams;
}

// A push of n_streams (camera: on sensor frames; round_stride: of a burst, else 0): nullptr and the tables it uses, or
// why it is refused.  The sensor records, the pixel formats and the binning belong to the camera forms alone: a push
// of pre-cropped frames does not look at them.  The formats and the binning go with sensor records only, and a round's
// base, k * round_stride, must be a number the kernels can form.
inline const char *bank_tables_for_push(const BankTables &b, int32_t n_streams, bool camera, int64_t round_stride, BankTablesUsed *out)
{
    BankTablesUsed u = {};
    if (bank_table_differs(b, kBankStreams, n_streams)) return "bank: n_streams differs from the array bound with aof_set_bank_streams";
    u.streams = static_cast<const aof_bank_stream *>(b.table[kBankStreams].array);
    if (camera) {
        if (bank_table_differs(b, kBankSensors, n_streams)) return "bank: n_streams differs from the array bound with aof_set_bank_sensors";
        u.sensors = static_cast<const aof_bank_sensor *>(b.table[kBankSensors].array);
        u.camera_bytes = b.camera_bytes;
        if (u.sensors && round_stride > INT64_MAX / AOF_BANK_BURST_MAX) return "bank burst: round_stride too large for sensor records";
        u.formats = static_cast<const uint8_t *>(b.table[kBankFormats].array);
        if (u.formats && !u.sensors) return "bank: pixel formats are bound (aof_set_bank_pixel_formats) without sensor records";
        if (bank_table_differs(b, kBankFormats, n_streams)) return "bank: n_streams differs from the array bound with aof_set_bank_pixel_formats";
        u.bins = static_cast<const uint8_t *>(b.table[kBankBins].array);
        if (u.bins && !u.sensors) return "bank: a binning is bound (aof_set_bank_binning) without sensor records";
        if (bank_table_differs(b, kBankBins, n_streams)) return "bank: n_streams differs from the array bound with aof_set_bank_binning";
    }
    *out = u;
    return nullptr;
}

// The IMU call of n_streams: the per-stream records give every stream its own identity; nothing else is looked at.
inline const char *bank_tables_for_imu(const BankTables &b, int32_t n_streams, const aof_bank_stream **streams)
{
    if (bank_table_differs(b, kBankStreams, n_streams)) return "imu: n_streams differs from the array bound with aof_set_bank_streams";
    *streams = static_cast<const aof_bank_stream *>(b.table[kBankStreams].array);
    return nullptr;
}

// The warp meshes (aof_set_bank_warps): a record of its own beside the tables -- an array of meshes, [S][ny][nx] nodes
// of the context's crop, is no per-stream table of fixed records, and a push with it bound takes another path
// (the tick with the warp inside it, or launch_warp in place of launch_ingest on the composed path) where a table only
// changes a kernel's argument.
struct BankWarps {
    const aof_warp_point *points;   // device memory of the caller's, or nullptr: nothing bound
    int32_t n_streams;
};

// The binding call: nullptr, or why it is refused -- the binding is then as it was.  A null array unbinds.
inline const char *bank_warps_bind(BankWarps *w, const aof_warp_point *points, int32_t n_streams)
{
    if (points && n_streams < 1) return "bank warps: an array needs n_streams >= 1";
    if (!aligned(points, 16)) return "bank warps: the array must be 16-byte aligned";
    w->points = points;
    w->n_streams = points ? n_streams : 0;
    return nullptr;
}

// A camera push of n_streams with the tables `u` it uses: nullptr and the meshes (or nullptr: nothing bound, the push
// runs as it always did), or why it is refused.
inline const char *bank_warps_for_push(const BankWarps &w, int32_t n_streams, const BankTablesUsed &u, const aof_warp_point **points)
{
    *points = nullptr;
    if (!w.points) return nullptr;
    if (w.n_streams != n_streams) return "bank: n_streams differs from the array bound with aof_set_bank_warps";
    if (u.bins) return "bank: a binning (aof_set_bank_binning) and warps (aof_set_bank_warps) are bound at the same time";
    *points = w.points;
    return nullptr;
}

// The kernels' sensor arguments of one round (base: bytes between the caller's d_camera and the round's first frame;
// sensors == nullptr: the kernels without the argument).
inline BankSensors bank_sensors_of_round(const BankTablesUsed &u, uint64_t base)
{
    return BankSensors{u.sensors, u.camera_bytes, base, u.formats, u.bins};
}

// ok: u8 per frame or nullptr, 1 where the record let the frame be read
inline IngestSensors ingest_sensors_of_round(const BankTablesUsed &u, uint64_t base, uint8_t *ok = nullptr)
{
    return IngestSensors{u.sensors, base, u.camera_bytes, ok, u.formats, u.bins};
}

// The stream bank's section of the context (a member of aof_ctx), and the one way to it for the host files that are
// built without the HIP runtime and so cannot see aof_ctx itself (defined beside the context's life, aof_capi.hip).
struct BankCtx {
    int path;                   // aof_set_bank_path: 0 the library chooses, 1 the one-launch tick kernel, 2 the composed path
    int last_path;              // aof_bank_last_path: 0 no push yet, 1 the last accepted push ran one-launch kernel(s), 2 the composed launches
    BankTables tables;          // aof_set_bank_streams / _sensors / _pixel_formats / _binning: the caller's per-stream arrays
    BankWarps warps;            // aof_set_bank_warps: the caller's meshes (beside the tables)
};
BankCtx &bank_ctx(aof_ctx *ctx);

}  // namespace aof
