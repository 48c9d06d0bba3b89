/*
 * emspec_napi.c — thin N-API (raw node_api.h, N-API >= 4) shim over the C ABI of
 * libemspec (include/emspec.h).  This is the process-internal FFI boundary of
 * renderer JS -> this shim -> libemspec -> HIP kernels.
 *
 * The reference ships no addon, binding.gyp or IPC schema (its source is private,
 * /root/reference/README.md:73); the only interface it names is the renderer call
 * computeSpectrogramColumn(audioFrame, fftSize, hop, reassign) (BASELINE.json).
 *
 * Ownership: typed-array memory is borrowed for the duration of a call only.
 * Errors: every failure throws a JS Error whose .code is the emspec_status name.
 * There is no CPU path: without a gfx950 device create() throws EMSPEC_ERR_NO_DEVICE.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/emspec.h"

#define NAPI_OK_OR_RETURN(env, call)                                     \
    do {                                                                 \
        if ((call) != napi_ok) {                                         \
            napi_throw_error((env), "EMSPEC_NAPI", "N-API call failed: " #call); \
            return NULL;                                                 \
        }                                                                \
    } while (0)

static const char* status_name(int rc) {
    switch (rc) {
        case EMSPEC_ERR_INVALID_ARG: return "EMSPEC_ERR_INVALID_ARG";
        case EMSPEC_ERR_NO_DEVICE: return "EMSPEC_ERR_NO_DEVICE";
        case EMSPEC_ERR_HIP: return "EMSPEC_ERR_HIP";
        case EMSPEC_ERR_OUT_OF_MEMORY: return "EMSPEC_ERR_OUT_OF_MEMORY";
        case EMSPEC_ERR_STATE: return "EMSPEC_ERR_STATE";
        case EMSPEC_ERR_COMM: return "EMSPEC_ERR_COMM";
        default: return "EMSPEC_ERR_UNKNOWN";
    }
}

static napi_value throw_status(napi_env env, emspec_engine* e, int rc) {
    napi_throw_error(env, status_name(rc), emspec_last_error(e));
    return NULL;
}

/* rows: the engine's row count, for output-size checks; wave: the array given to setWaveOut, referenced while it is set;
 * level / cross: likewise the arrays given to setLevelOut / setCrossOut; live_peaks / live_wave: those given to setLivePeaks /
 * setLiveWave; live_level / live_cross: setLiveLevel / setLiveCross */
typedef struct { emspec_engine* e; int32_t rows; napi_ref wave, level, cross, live_peaks, live_wave, live_level, live_cross; } handle_t;

static void drop_ref(napi_env env, napi_ref* r) {
    if (*r) { napi_delete_reference(env, *r); *r = NULL; }
}
static void drop_wave(napi_env env, handle_t* h) {   /* ... and the level meters' arrays: what the batch calls also fill */
    drop_ref(env, &h->wave);
    drop_ref(env, &h->level);
    drop_ref(env, &h->cross);
}
static void drop_live(napi_env env, handle_t* h) {   /* the arrays the live calls also fill */
    drop_ref(env, &h->live_peaks);
    drop_ref(env, &h->live_wave);
    drop_ref(env, &h->live_level);
    drop_ref(env, &h->live_cross);
}
static void finalize_handle(napi_env env, void* data, void* hint) {
    (void)hint;
    handle_t* h = (handle_t*)data;
    if (h) { if (h->e) emspec_destroy(h->e); drop_wave(env, h); drop_live(env, h); free(h); }
}

static int get_number_prop(napi_env env, napi_value obj, const char* name, double* out) {
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
    napi_value v;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return 0;
    return napi_get_value_double(env, v, out) == napi_ok;
}

static handle_t* get_handle(napi_env env, napi_value v) {
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((handle_t*)p)->e) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "not a live emspec engine handle");
        return NULL;
    }
    return (handle_t*)p;
}

/* typed array of the wanted element type, or NULL data when the value is undefined/null */
static int get_typed(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len, int optional) {
    *data = NULL; *len = 0;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (optional && (t == napi_undefined || t == napi_null)) return 1;
    bool is = false;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return 0;
    napi_typedarray_type ty; napi_value ab; size_t off;
    if (napi_get_typedarray_info(env, v, &ty, len, data, &ab, &off) != napi_ok) return 0;
    return ty == want;
}

/* create(config) -> external */
static napi_value Create(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    emspec_config cfg;
    emspec_default_config(&cfg);
    if (argc >= 1) {
        napi_valuetype t;
        NAPI_OK_OR_RETURN(env, napi_typeof(env, argv[0], &t));
        if (t == napi_object) {
            double d;
            if (get_number_prop(env, argv[0], "device", &d)) cfg.device = (int32_t)d;
            if (get_number_prop(env, argv[0], "rows", &d)) cfg.rows = (int32_t)d;
            if (get_number_prop(env, argv[0], "sampleRate", &d)) cfg.sample_rate = (float)d;
            if (get_number_prop(env, argv[0], "fminHz", &d)) cfg.fmin_hz = (float)d;
            if (get_number_prop(env, argv[0], "fmaxHz", &d)) cfg.fmax_hz = (float)d;
            if (get_number_prop(env, argv[0], "gain", &d)) cfg.gain = (float)d;
            if (get_number_prop(env, argv[0], "dbTop", &d)) cfg.db_top = (float)d;
            if (get_number_prop(env, argv[0], "dbRange", &d)) cfg.db_range = (float)d;
            if (get_number_prop(env, argv[0], "gateDb", &d)) cfg.gate_db = (float)d;
            if (get_number_prop(env, argv[0], "powerFloor", &d)) cfg.power_floor = (float)d;
            /* exact: true -> EMSPEC_MODE_EXACT (binary64 + 64-bit fixed-point histogram: indices equal to a float64
             * implementation, reproducible bytes); default EMSPEC_MODE_FAST */
            napi_value ex; bool has = false, on = false;
            if (napi_has_named_property(env, argv[0], "exact", &has) == napi_ok && has &&
                napi_get_named_property(env, argv[0], "exact", &ex) == napi_ok &&
                napi_coerce_to_bool(env, ex, &ex) == napi_ok && napi_get_value_bool(env, ex, &on) == napi_ok && on)
                cfg.mode = EMSPEC_MODE_EXACT;
        }
    }
    emspec_engine* e = NULL;
    int rc = emspec_create(&cfg, &e);
    if (rc != EMSPEC_OK) return throw_status(env, NULL, rc);
    if (emspec_mode(e) != cfg.mode) {   /* a library that ignores the mode field must not pass for an exact engine */
        emspec_destroy(e);
        napi_throw_error(env, "EMSPEC_ERR_STATE", "the library did not honour the requested arithmetic mode");
        return NULL;
    }
    handle_t* h = (handle_t*)malloc(sizeof(handle_t));
    if (!h) { emspec_destroy(e); napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "malloc"); return NULL; }
    h->e = e;
    h->rows = cfg.rows;
    h->wave = h->level = h->cross = NULL;
    h->live_peaks = h->live_wave = h->live_level = h->live_cross = NULL;
    napi_value ext;
    if (napi_create_external(env, h, finalize_handle, NULL, &ext) != napi_ok) {
        finalize_handle(env, h, NULL);
        napi_throw_error(env, "EMSPEC_NAPI", "napi_create_external failed");
        return NULL;
    }
    return ext;
}

static napi_value Destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    void* p = NULL;
    if (argc >= 1 && napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
        handle_t* h = (handle_t*)p;
        if (h->e) { emspec_destroy(h->e); h->e = NULL; }
        drop_wave(env, h);
        drop_live(env, h);
    }
    return NULL;
}

static napi_value Rows(napi_env env, napi_callback_info info) {
    /* rows(config) -> rows the engine would use (defaults applied) */
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    emspec_config cfg; emspec_default_config(&cfg);
    double d;
    if (argc >= 1 && get_number_prop(env, argv[0], "rows", &d)) cfg.rows = (int32_t)d;
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int32(env, cfg.rows, &r));
    return r;
}

/* column(handle, frame:Float32Array, fftSize, hop, reassign, outDb?:Float32Array, outRgba?:Uint8Array) -> column index (-1 while priming) */
static napi_value Column(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "column(handle, frame, fftSize, hop, reassign[, outDb, outRgba])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* frame; size_t flen;
    if (!get_typed(env, argv[1], napi_float32_array, &frame, &flen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "audioFrame must be a Float32Array"); return NULL; }
    int32_t n, hop; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[4], &argv[4]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[4], &reassign));
    if ((size_t)n != flen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "audioFrame.length must equal fftSize"); return NULL; }
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0;
    if (argc > 5 && !get_typed(env, argv[5], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 6 && !get_typed(env, argv[6], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    int32_t rows = db ? (int32_t)dblen : (int32_t)(rgbalen / 4);
    if (rgba && db && rgbalen != 4 * dblen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba.length must be 4*outDb.length"); return NULL; }
    int64_t col = -1;
    int rc = emspec_column(h->e, (const float*)frame, n, hop, reassign ? 1 : 0, (float*)db, (uint8_t*)rgba, rows, &col);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, col, &r));
    return r;
}

/* flush(handle, outDb?, outRgba?) -> column index */
static napi_value Flush(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "flush(handle, outDb[, outRgba])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0;
    if (!get_typed(env, argv[1], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 2 && !get_typed(env, argv[2], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    int32_t rows = db ? (int32_t)dblen : (int32_t)(rgbalen / 4);
    int64_t col = -1;
    int rc = emspec_column_flush(h->e, (float*)db, (uint8_t*)rgba, rows, &col);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, col, &r));
    return r;
}

/* pushColumns(handle, count, fftSize, hop, reassign) -> columns a block of `count` samples will complete */
static napi_value PushColumns(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pushColumns(handle, count, fftSize, hop, reassign)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int64_t count; int32_t n, hop; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &count));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[4], &argv[4]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[4], &reassign));
    const int64_t k = emspec_push_columns(h->e, count, n, hop, reassign ? 1 : 0);
    if (k < 0) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "invalid count / fftSize / hop"); return NULL; }
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, k, &r));
    return r;
}

/* push(handle, samples:Float32Array, fftSize, hop, reassign, rows, outDb?:Float32Array(k*rows), outRgba?:Uint8Array(4*k*rows))
 * -> absolute index of the first completed column (-1 when the block completed none) */
static napi_value Push(napi_env env, napi_callback_info info) {
    size_t argc = 8; napi_value argv[8];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 6) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "push(handle, samples, fftSize, hop, reassign, rows[, outDb, outRgba])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* smp; size_t slen;
    if (!get_typed(env, argv[1], napi_float32_array, &smp, &slen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "samples must be a Float32Array"); return NULL; }
    int32_t n, hop, rows; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[4], &argv[4]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[4], &reassign));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &rows));
    if (rows < 1) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "rows must be positive"); return NULL; }
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0;
    if (argc > 6 && !get_typed(env, argv[6], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 7 && !get_typed(env, argv[7], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    int64_t room = INT64_MAX;   /* columns the smaller output can hold */
    if (db) room = (int64_t)(dblen / (size_t)rows);
    if (rgba && (int64_t)(rgbalen / (4 * (size_t)rows)) < room) room = (int64_t)(rgbalen / (4 * (size_t)rows));
    int64_t count = 0, first = -1;
    int rc = emspec_push_samples(h->e, (const float*)smp, (int64_t)slen, n, hop, reassign ? 1 : 0, (float*)db, (uint8_t*)rgba,
                                 rows, room, &count, &first);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, first, &r));
    return r;
}

/* warpedEdges(rows, fminHz, fmaxHz, lowEndBoost, freqScale) -> Float32Array(rows+1)  (emspec_warped_edges_hz) */
static napi_value WarpedEdges(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "warpedEdges(rows, fminHz, fmaxHz, lowEndBoost, freqScale)"); return NULL; }
    int32_t rows; double a[4];
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[0], &rows));
    for (int i = 0; i < 4; ++i) NAPI_OK_OR_RETURN(env, napi_get_value_double(env, argv[1 + i], &a[i]));
    if (rows < 1 || rows > (1 << 20)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "rows out of range"); return NULL; }
    napi_value ab, ta; void* data = NULL;
    NAPI_OK_OR_RETURN(env, napi_create_arraybuffer(env, (size_t)(rows + 1) * 4, &data, &ab));
    if (emspec_warped_edges_hz(rows, (float)a[0], (float)a[1], (float)a[2], (float)a[3], (float*)data) != EMSPEC_OK) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "need 0 < fminHz < fmaxHz, lowEndBoost > 0, freqScale > 0");
        return NULL;
    }
    NAPI_OK_OR_RETURN(env, napi_create_typedarray(env, napi_float32_array, (size_t)rows + 1, ab, 0, &ta));
    return ta;
}

/* referenceColormap(brightness) -> Uint8Array(1024)  (emspec_make_colormap) */
static napi_value ReferenceColormap(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    double b = 0.5;
    if (argc >= 1) NAPI_OK_OR_RETURN(env, napi_get_value_double(env, argv[0], &b));
    napi_value ab, ta; void* data = NULL;
    NAPI_OK_OR_RETURN(env, napi_create_arraybuffer(env, 1024, &data, &ab));
    if (emspec_make_colormap((float)b, (uint8_t*)data) != EMSPEC_OK) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "brightness must be >= 0"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_create_typedarray(env, napi_uint8_array, 1024, ab, 0, &ta));
    return ta;
}

static napi_value Reset(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int rc = emspec_reset(h->e);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* batch(handle, pcm:Float32Array(S*L), S, L, fftSize, hop, reassign, outDb?, outRgba?, outIndex?) -> columns per stream */
/* columns per stream a batch entry DELIVERS for `columns` full-rate ones: the engine's time reduction (emspec_set_time_reduce)
 * collapses groups of that many columns into one; every output array of the batch calls below is sized by it */
static int64_t out_columns(const handle_t* h, int64_t columns) {
    return columns > 0 ? emspec_reduced_columns(columns, emspec_time_reduce(h->e)) : columns;
}

static napi_value Batch(napi_env env, napi_callback_info info) {
    size_t argc = 10; napi_value argv[10];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 8) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batch(handle, pcm, S, L, fftSize, hop, reassign, outDb[, outRgba, outIndex])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, n, hop; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[6], &argv[6]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[6], &reassign));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    emspec_out out; memset(&out, 0, sizeof(out));
    size_t l0 = 0, l1 = 0, l2 = 0; void *p0 = NULL, *p1 = NULL, *p2 = NULL;
    if (!get_typed(env, argv[7], napi_float32_array, &p0, &l0, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 8 && !get_typed(env, argv[8], napi_uint8_array, &p1, &l1, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 9 && !get_typed(env, argv[9], napi_uint8_array, &p2, &l2, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array"); return NULL; }
    int64_t C = out_columns(h, emspec_num_columns(L, n, hop));
    /* sizes are checked against rows implied by the first output given */
    size_t cells = 0;
    if (p0) cells = l0; else if (p1) cells = l1 / 4; else if (p2) cells = l2;
    /* emspec_batch writes S*columns*rows cells with the ENGINE's row count: anything else would overrun the array */
    if (C <= 0 || cells != (size_t)S * (size_t)C * (size_t)h->rows || (p1 && l1 != 4 * cells) || (p2 && l2 != cells) || (p0 && l0 != cells)) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "output arrays must hold exactly S*columns*rows cells, rows = the engine's row count (rgba: 4 bytes per cell)");
        return NULL;
    }
    out.db = (float*)p0; out.rgba = (uint8_t*)p1; out.index = (uint8_t*)p2;
    int rc = emspec_batch(h->e, (const float*)pcm, S, L, n, hop, reassign ? 1 : 0, &out);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}

/* batchMultires(handle, pcm:Float32Array(S*L), S, L, lowFftSize, fftSize, hop, splitRow, reassign, outDb[, outRgba, outIndex])
 * -> columns.  emspec_batch_multires: lowFftSize below splitRow, fftSize from it up, on one column grid (synchronous). */
static napi_value BatchMultires(napi_env env, napi_callback_info info) {
    size_t argc = 12; napi_value argv[12];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 10) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchMultires(handle, pcm, S, L, lowFftSize, fftSize, hop, splitRow, reassign, outDb[, outRgba, outIndex])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, nl, nh, hop, split; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &nl));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &nh));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &hop));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &split));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[8], &argv[8]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[8], &reassign));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    /* C <= 0: a shape (or L) the library rejects, with a message naming the rule, before it touches any output */
    const int64_t C = out_columns(h, emspec_multires_columns(L, nl, nh, hop));
    size_t l0 = 0, l1 = 0, l2 = 0; void *p0 = NULL, *p1 = NULL, *p2 = NULL;
    if (!get_typed(env, argv[9], napi_float32_array, &p0, &l0, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 10 && !get_typed(env, argv[10], napi_uint8_array, &p1, &l1, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 11 && !get_typed(env, argv[11], napi_uint8_array, &p2, &l2, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array"); return NULL; }
    size_t cells = 0;
    if (p0) cells = l0; else if (p1) cells = l1 / 4; else if (p2) cells = l2;
    if (C > 0 && (cells != (size_t)S * (size_t)C * (size_t)h->rows || (p1 && l1 != 4 * cells) || (p2 && l2 != cells) || (p0 && l0 != cells))) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "output arrays must hold exactly S*columns*rows cells, rows = the engine's row count (rgba: 4 bytes per cell)");
        return NULL;
    }
    emspec_out out; memset(&out, 0, sizeof(out));
    out.db = (float*)p0; out.rgba = (uint8_t*)p1; out.index = (uint8_t*)p2;
    int rc = emspec_batch_multires(h->e, (const float*)pcm, S, L, nl, nh, hop, split, reassign ? 1 : 0, &out);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}

/* An Int32Array of 1..8 values (FFT sizes or split rows of the multi-band batch) -> vals[8], *count; the library judges the count. */
static int get_int32_list(napi_env env, napi_value v, int32_t* vals, int32_t* count) {
    void* p; size_t len;
    if (!get_typed(env, v, napi_int32_array, &p, &len, 0) || len > 8) return 0;
    memset(vals, 0, 8 * sizeof(int32_t));
    if (len) memcpy(vals, p, len * sizeof(int32_t));
    *count = (int32_t)len;
    return 1;
}

/* batchMultiband(handle, pcm:Float32Array(S*L), S, L, fftSizes:Int32Array(K), splitRows:Int32Array(K-1), hop, reassign, outDb[, outRgba,
 * outIndex]) -> columns.  emspec_batch_multiband: fftSizes[k] for the rows from splitRows[k-1] up, on one column grid (synchronous). */
static napi_value BatchMultiband(napi_env env, napi_callback_info info) {
    size_t argc = 11; napi_value argv[11];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 9) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchMultiband(handle, pcm, S, L, fftSizes, splitRows, hop, reassign, outDb[, outRgba, outIndex])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, hop, K = 0, nsplit = 0, n[8], split[8]; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    if (!get_int32_list(env, argv[4], n, &K) || !get_int32_list(env, argv[5], split, &nsplit)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "fftSizes and splitRows must be Int32Arrays of at most 8 values"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[7], &argv[7]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[7], &reassign));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    if (K >= 2 && K <= 4 && nsplit != K - 1) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "splitRows must hold one row fewer than fftSizes"); return NULL; }
    /* C <= 0: a shape (or L) the library rejects, with a message naming the rule, before it touches any output */
    const int64_t C = out_columns(h, emspec_multiband_columns(L, K, n, hop));
    size_t l0 = 0, l1 = 0, l2 = 0; void *p0 = NULL, *p1 = NULL, *p2 = NULL;
    if (!get_typed(env, argv[8], napi_float32_array, &p0, &l0, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 9 && !get_typed(env, argv[9], napi_uint8_array, &p1, &l1, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 10 && !get_typed(env, argv[10], napi_uint8_array, &p2, &l2, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array"); return NULL; }
    size_t cells = 0;
    if (p0) cells = l0; else if (p1) cells = l1 / 4; else if (p2) cells = l2;
    if (C > 0 && (cells != (size_t)S * (size_t)C * (size_t)h->rows || (p1 && l1 != 4 * cells) || (p2 && l2 != cells) || (p0 && l0 != cells))) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "output arrays must hold exactly S*columns*rows cells, rows = the engine's row count (rgba: 4 bytes per cell)");
        return NULL;
    }
    emspec_out out; memset(&out, 0, sizeof(out));
    out.db = (float*)p0; out.rgba = (uint8_t*)p1; out.index = (uint8_t*)p2;
    int rc = emspec_batch_multiband(h->e, (const float*)pcm, S, L, K, n, split, hop, reassign ? 1 : 0, &out);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}

/* batchPacked(handle, pcm:Float32Array(S*L), S, L, fftSize, hop, reassign, wire:Uint8Array, offsets:Float64Array(S+1)) -> columns
 * per stream.  emspec_batch_packed: the palette-index columns cross PCIe as one lossless wire image per stream; stream s
 * is wire.subarray(offsets[s], offsets[s+1]) (offsets as doubles: exact below 2^53). */
static napi_value BatchPacked(napi_env env, napi_callback_info info) {
    size_t argc = 9; napi_value argv[9];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 9) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchPacked(handle, pcm, S, L, fftSize, hop, reassign, wire, offsets)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, n, hop; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[6], &argv[6]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[6], &reassign));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    void *wire = NULL, *offs = NULL; size_t wlen = 0, olen = 0;
    if (!get_typed(env, argv[7], napi_uint8_array, &wire, &wlen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "wire must be a Uint8Array"); return NULL; }
    if (!get_typed(env, argv[8], napi_float64_array, &offs, &olen, 0) || olen != (size_t)S + 1) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "offsets must be a Float64Array(S + 1)"); return NULL;
    }
    int64_t* o64 = (int64_t*)malloc(sizeof(int64_t) * ((size_t)S + 1));
    if (!o64) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "out of host memory"); return NULL; }
    int rc = emspec_batch_packed(h->e, (const float*)pcm, S, L, n, hop, reassign ? 1 : 0, (uint8_t*)wire, (int64_t)wlen, o64);
    if (rc == EMSPEC_OK) for (int32_t i = 0; i <= S; ++i) ((double*)offs)[i] = (double)o64[i];
    free(o64);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, out_columns(h, emspec_num_columns(L, n, hop)), &r));
    return r;
}

/* wireUnpack(image:Uint8Array, columns, rows, out:Uint8Array(columns*rows)): emspec_wire_unpack_host (no device, no engine) */
static napi_value WireUnpack(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "wireUnpack(image, columns, rows, out)"); return NULL; }
    void *img = NULL, *out = NULL; size_t ilen = 0, olen = 0;
    int64_t columns; int32_t rows;
    if (!get_typed(env, argv[0], napi_uint8_array, &img, &ilen, 0) || !get_typed(env, argv[3], napi_uint8_array, &out, &olen, 0)) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "image and out must be Uint8Arrays"); return NULL;
    }
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &columns));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &rows));
    if (columns < 1 || rows < 1 || olen != (size_t)columns * (size_t)rows) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "out.length must equal columns*rows"); return NULL; }
    if (emspec_wire_unpack_host((const uint8_t*)img, (int64_t)ilen, columns, rows, (uint8_t*)out) != EMSPEC_OK) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "the wire image does not match (columns, rows) or is damaged"); return NULL;
    }
    return NULL;
}

static napi_value WireBound(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int64_t columns = 0; int32_t rows = 0;
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "wireBound(columns, rows)"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[0], &columns));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &rows));
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_wire_bound(columns, rows), &r));
    return r;
}

/* batchAsync(handle, pcm, S, L, fftSize, hop, reassign, outDb?, outRgba?, outIndex?) -> Promise<columns>
 * Same as batch() but the work runs on the libuv thread pool (napi_create_async_work), so the
 * renderer's JS thread is not blocked for the duration of a large batch.  The typed arrays are
 * kept alive by references until completion; the caller must not touch them, nor call into the
 * same engine, before the promise settles (an engine is not thread-safe). */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[4];
    emspec_engine* e;
    const float* pcm;
    emspec_out out;
    int32_t S, n, hop, reassign;
    int64_t L, C;
    int rc;
    char msg[256];
} batch_job;

static void batch_execute(napi_env env, void* data) {
    (void)env;
    batch_job* j = (batch_job*)data;
    j->rc = emspec_batch(j->e, j->pcm, j->S, j->L, j->n, j->hop, j->reassign, &j->out);
    if (j->rc != EMSPEC_OK) { strncpy(j->msg, emspec_last_error(j->e), sizeof(j->msg) - 1); j->msg[sizeof(j->msg) - 1] = 0; }
}

static void batch_complete(napi_env env, napi_status status, void* data) {
    batch_job* j = (batch_job*)data;
    for (int i = 0; i < 4; ++i) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
    if (status == napi_ok && j->rc == EMSPEC_OK) {
        napi_value v; napi_create_int64(env, j->C, &v);
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value code, msg, err;
        napi_create_string_utf8(env, status == napi_ok ? status_name(j->rc) : "EMSPEC_NAPI", NAPI_AUTO_LENGTH, &code);
        napi_create_string_utf8(env, status == napi_ok ? j->msg : "async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, code, msg, &err);
        napi_reject_deferred(env, j->deferred, err);
    }
    napi_delete_async_work(env, j->work);
    free(j);
}

static napi_value BatchAsync(napi_env env, napi_callback_info info) {
    size_t argc = 10; napi_value argv[10];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 8) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchAsync(handle, pcm, S, L, fftSize, hop, reassign, outDb[, outRgba, outIndex])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, n, hop; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[6], &argv[6]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[6], &reassign));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    size_t l0 = 0, l1 = 0, l2 = 0; void *p0 = NULL, *p1 = NULL, *p2 = NULL;
    if (!get_typed(env, argv[7], napi_float32_array, &p0, &l0, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 8 && !get_typed(env, argv[8], napi_uint8_array, &p1, &l1, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 9 && !get_typed(env, argv[9], napi_uint8_array, &p2, &l2, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array"); return NULL; }
    int64_t C = out_columns(h, emspec_num_columns(L, n, hop));
    size_t cells = p0 ? l0 : (p1 ? l1 / 4 : l2);
    if (C <= 0 || cells != (size_t)S * (size_t)C * (size_t)h->rows || (p1 && l1 != 4 * cells) || (p2 && l2 != cells) || (p0 && l0 != cells)) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "output arrays must hold exactly S*columns*rows cells, rows = the engine's row count (rgba: 4 bytes per cell)");
        return NULL;
    }
    batch_job* j = (batch_job*)calloc(1, sizeof(batch_job));
    if (!j) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "calloc"); return NULL; }
    j->e = h->e; j->pcm = (const float*)pcm; j->S = S; j->L = L; j->n = n; j->hop = hop; j->reassign = reassign ? 1 : 0; j->C = C;
    j->out.db = (float*)p0; j->out.rgba = (uint8_t*)p1; j->out.index = (uint8_t*)p2;
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) { free(j); napi_throw_error(env, "EMSPEC_NAPI", "napi_create_promise"); return NULL; }
    napi_create_reference(env, argv[1], 1, &j->refs[0]);                       /* keep the buffers alive */
    if (p0) napi_create_reference(env, argv[7], 1, &j->refs[1]);
    if (p1) napi_create_reference(env, argv[8], 1, &j->refs[2]);
    if (p2) napi_create_reference(env, argv[9], 1, &j->refs[3]);
    napi_create_string_utf8(env, "emspec.batchAsync", NAPI_AUTO_LENGTH, &name);
    if (napi_create_async_work(env, NULL, name, batch_execute, batch_complete, j, &j->work) != napi_ok ||
        napi_queue_async_work(env, j->work) != napi_ok) {
        for (int i = 0; i < 4; ++i) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
        free(j);
        napi_throw_error(env, "EMSPEC_NAPI", "could not queue async work");
        return NULL;
    }
    return promise;
}

/* batchPackedAsync(handle, pcm, S, L, fftSize, hop, reassign, wire, offsets:Float64Array(S+1)) -> Promise<columns>: batchPacked on the
 * libuv thread pool.  The typed arrays are kept alive by references; the caller touches neither them nor the engine before
 * the promise settles. */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[3];
    emspec_engine* e;
    const float* pcm;
    uint8_t* wire;
    int64_t wire_len;
    double* offs;
    int64_t* o64;
    int32_t S, n, hop, reassign;
    int64_t L, C;
    int rc;
    char msg[256];
} packed_job;

static void packed_execute(napi_env env, void* data) {
    (void)env;
    packed_job* j = (packed_job*)data;
    j->rc = emspec_batch_packed(j->e, j->pcm, j->S, j->L, j->n, j->hop, j->reassign, j->wire, j->wire_len, j->o64);
    if (j->rc != EMSPEC_OK) { strncpy(j->msg, emspec_last_error(j->e), sizeof(j->msg) - 1); j->msg[sizeof(j->msg) - 1] = 0; }
}

static void packed_complete(napi_env env, napi_status status, void* data) {
    packed_job* j = (packed_job*)data;
    if (status == napi_ok && j->rc == EMSPEC_OK) for (int32_t i = 0; i <= j->S; ++i) j->offs[i] = (double)j->o64[i];   /* (the array is still referenced) */
    for (int i = 0; i < 3; ++i) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
    if (status == napi_ok && j->rc == EMSPEC_OK) {
        napi_value v; napi_create_int64(env, j->C, &v);
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value code, msg, err;
        napi_create_string_utf8(env, status == napi_ok ? status_name(j->rc) : "EMSPEC_NAPI", NAPI_AUTO_LENGTH, &code);
        napi_create_string_utf8(env, status == napi_ok ? j->msg : "async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, code, msg, &err);
        napi_reject_deferred(env, j->deferred, err);
    }
    napi_delete_async_work(env, j->work);
    free(j->o64);
    free(j);
}

static napi_value BatchPackedAsync(napi_env env, napi_callback_info info) {
    size_t argc = 9; napi_value argv[9];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 9) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchPackedAsync(handle, pcm, S, L, fftSize, hop, reassign, wire, offsets)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, n, hop; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[6], &argv[6]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[6], &reassign));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    void *wire = NULL, *offs = NULL; size_t wlen = 0, olen = 0;
    if (!get_typed(env, argv[7], napi_uint8_array, &wire, &wlen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "wire must be a Uint8Array"); return NULL; }
    if (!get_typed(env, argv[8], napi_float64_array, &offs, &olen, 0) || olen != (size_t)S + 1) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "offsets must be a Float64Array(S + 1)"); return NULL;
    }
    packed_job* j = (packed_job*)calloc(1, sizeof(packed_job));
    if (j) j->o64 = (int64_t*)malloc(sizeof(int64_t) * ((size_t)S + 1));
    if (!j || !j->o64) { free(j); napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "out of host memory"); return NULL; }
    j->e = h->e; j->pcm = (const float*)pcm; j->S = S; j->L = L; j->n = n; j->hop = hop; j->reassign = reassign ? 1 : 0;
    j->C = out_columns(h, emspec_num_columns(L, n, hop)); j->wire = (uint8_t*)wire; j->wire_len = (int64_t)wlen; j->offs = (double*)offs;
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) { free(j->o64); free(j); napi_throw_error(env, "EMSPEC_NAPI", "napi_create_promise"); return NULL; }
    napi_create_reference(env, argv[1], 1, &j->refs[0]);
    napi_create_reference(env, argv[7], 1, &j->refs[1]);
    napi_create_reference(env, argv[8], 1, &j->refs[2]);
    napi_create_string_utf8(env, "emspec.batchPackedAsync", NAPI_AUTO_LENGTH, &name);
    if (napi_create_async_work(env, NULL, name, packed_execute, packed_complete, j, &j->work) != napi_ok ||
        napi_queue_async_work(env, j->work) != napi_ok) {
        for (int i = 0; i < 3; ++i) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
        free(j->o64); free(j);
        napi_throw_error(env, "EMSPEC_NAPI", "could not queue async work");
        return NULL;
    }
    return promise;
}

/* ---- live multi-stream streaming (emspec_columns / emspec_push_samples_multi): S streams per call, one launch ---- */

/* optional Float64Array(S) that receives int64 values (column indices / counts: exact in a double) */
static int get_f64_out(napi_env env, napi_value v, size_t want, double** out) {
    void* d = NULL; size_t len = 0;
    *out = NULL;
    if (!get_typed(env, v, napi_float64_array, &d, &len, 1)) return 0;
    if (d && len != want) return 0;
    *out = (double*)d;
    return 1;
}

/* columns(handle, frames:Float32Array(S*fftSize), S, fftSize, hop, reassign, outDb?:Float32Array(S*rows),
 *         outRgba?:Uint8Array(4*S*rows), outColumns?:Float64Array(S)) : one frame of each of S streams -> their finished columns */
/* Optional trailing pair of the live calls (columns, pushMulti): nHigh > 0 makes the call the multi-resolution one - fftSize is
 * then n_low, and the rows from splitRow up come from nHigh (emspec_columns_multires / emspec_push_samples_multires). */
static bool get_multires_pair(napi_env env, size_t argc, napi_value* argv, size_t at, int32_t* n_high, int32_t* split) {
    *n_high = 0; *split = 0;
    if (argc < at + 2) return true;
    return napi_get_value_int32(env, argv[at], n_high) == napi_ok && napi_get_value_int32(env, argv[at + 1], split) == napi_ok;
}

/* Optional trailing pair behind that one: fftSizes:Int32Array(K), splitRows:Int32Array(K-1) make the call the multi-band one
 * (emspec_columns_multiband / emspec_push_samples_multiband / _pcm_multiband); fftSize is then fftSizes[0] and the pair before it
 * is ignored.  *K = 0: absent.  The library judges the sizes, the split rows and K itself. */
static bool get_bands(napi_env env, size_t argc, napi_value* argv, size_t at, int32_t* K, int32_t* n, int32_t* split) {
    *K = 0;
    if (argc < at + 2) return true;
    int32_t nsplit = 0;
    if (!get_int32_list(env, argv[at], n, K) || !get_int32_list(env, argv[at + 1], split, &nsplit)) return false;
    return *K < 1 || nsplit == *K - 1;
}
#define BANDS_OR_THROW(at) \
    int32_t K, bn[8], bsplit[8]; \
    if (!get_bands(env, argc, argv, (at), &K, bn, bsplit)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "fftSizes and splitRows must be Int32Arrays of at most 8 values, splitRows one fewer than fftSizes"); return NULL; }

static napi_value Columns(napi_env env, napi_callback_info info) {
    size_t argc = 13; napi_value argv[13];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 6) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "columns(handle, frames, S, fftSize, hop, reassign[, outDb, outRgba, outColumns])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* fr; size_t flen;
    if (!get_typed(env, argv[1], napi_float32_array, &fr, &flen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "frames must be a Float32Array"); return NULL; }
    int32_t S, n, hop; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[5], &argv[5]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[5], &reassign));
    if (S < 1 || n < 1 || (size_t)S * (size_t)n != flen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "frames.length must equal S*fftSize"); return NULL; }
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0; double* ocol = NULL;
    if (argc > 6 && !get_typed(env, argv[6], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 7 && !get_typed(env, argv[7], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 8 && !get_f64_out(env, argv[8], (size_t)S, &ocol)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outColumns must be a Float64Array(S)"); return NULL; }
    int32_t n_high, split;
    if (!get_multires_pair(env, argc, argv, 9, &n_high, &split)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "nHigh and splitRow must be integers"); return NULL; }
    BANDS_OR_THROW(11)
    const size_t cells = (size_t)S * (size_t)h->rows;
    if ((db && dblen != cells) || (rgba && rgbalen != 4 * cells)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must hold S*rows floats, outRgba 4*S*rows bytes (rows = the engine's row count)"); return NULL; }
    int64_t* c64 = ocol ? (int64_t*)malloc((size_t)S * sizeof(int64_t)) : NULL;
    if (ocol && !c64) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "malloc"); return NULL; }
    int rc = K > 0 ? emspec_columns_multiband(h->e, (const float*)fr, S, K, bn, bsplit, hop, reassign ? 1 : 0, (float*)db, (uint8_t*)rgba, h->rows, c64)
           : n_high > 0 ? emspec_columns_multires(h->e, (const float*)fr, S, n, n_high, hop, split, reassign ? 1 : 0, (float*)db, (uint8_t*)rgba, h->rows, c64)
                        : emspec_columns(h->e, (const float*)fr, S, n, hop, reassign ? 1 : 0, (float*)db, (uint8_t*)rgba, h->rows, c64);
    if (rc == EMSPEC_OK && ocol) for (int32_t s = 0; s < S; ++s) ocol[s] = (double)c64[s];
    free(c64);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* columnsFlush(handle, outDb?, outRgba?, outColumns?:Float64Array(S)): every stream with pending columns emits its next one */
static napi_value ColumnsFlush(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "columnsFlush(handle[, outDb, outRgba, outColumns])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    const int32_t S = emspec_live_streams(h->e);
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0; double* ocol = NULL;
    if (argc > 1 && !get_typed(env, argv[1], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 2 && !get_typed(env, argv[2], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 3 && !get_f64_out(env, argv[3], (size_t)S, &ocol)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outColumns must be a Float64Array(S)"); return NULL; }
    const size_t cells = (size_t)S * (size_t)h->rows;
    if ((db && dblen != cells) || (rgba && rgbalen != 4 * cells)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must hold S*rows floats, outRgba 4*S*rows bytes (S = the live session's streams)"); return NULL; }
    int64_t* c64 = (ocol && S > 0) ? (int64_t*)malloc((size_t)S * sizeof(int64_t)) : NULL;
    int rc = emspec_columns_flush(h->e, (float*)db, (uint8_t*)rgba, h->rows, c64);
    if (rc == EMSPEC_OK && ocol && c64) for (int32_t s = 0; s < S; ++s) ocol[s] = (double)c64[s];
    free(c64);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* pushColumnsMulti(handle, count, fftSize, hop, reassign[, nHigh[, fftSizes]]) -> the largest per-stream column count a block of `count` samples completes */
static napi_value PushColumnsMulti(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pushColumnsMulti(handle, count, fftSize, hop, reassign[, nHigh])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int64_t count; int32_t n, hop; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &count));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[4], &argv[4]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[4], &reassign));
    int32_t n_high = 0;   /* > 0: the multi-resolution session's count (fftSize = n_low) */
    if (argc > 5) NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &n_high));
    int32_t K = 0, bn[8];   /* fftSizes:Int32Array: the multi-band session's count */
    if (argc > 6 && !get_int32_list(env, argv[6], bn, &K)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "fftSizes must be an Int32Array of at most 8 values"); return NULL; }
    const int64_t k = K > 0 ? emspec_push_columns_multiband(h->e, count, K, bn, hop, reassign ? 1 : 0)
                    : n_high > 0 ? emspec_push_columns_multires(h->e, count, n, n_high, hop, reassign ? 1 : 0)
                                 : emspec_push_columns_multi(h->e, count, n, hop, reassign ? 1 : 0);
    /* (a multi-band shape that is not accepted: -1, and the push call that follows names the rule it breaks) */
    if (k < 0 && K == 0) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "invalid count / fftSize / hop"); return NULL; }
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, k, &r));
    return r;
}

/* pushMulti(handle, samples:Float32Array(S*count), S, fftSize, hop, reassign, maxColumns, outDb?:Float32Array(S*maxColumns*rows),
 *           outRgba?:Uint8Array(4*S*maxColumns*rows), outCounts?:Float64Array(S), outFirst?:Float64Array(S)) */
static napi_value PushMulti(napi_env env, napi_callback_info info) {
    size_t argc = 15; napi_value argv[15];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 7) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pushMulti(handle, samples, S, fftSize, hop, reassign, maxColumns[, outDb, outRgba, outCounts, outFirst])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* smp; size_t slen;
    if (!get_typed(env, argv[1], napi_float32_array, &smp, &slen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "samples must be a Float32Array"); return NULL; }
    int32_t S, n, hop; int64_t maxc; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[5], &argv[5]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[5], &reassign));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[6], &maxc));
    if (S < 1 || slen % (size_t)S != 0) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "samples.length must be a multiple of S"); return NULL; }
    if (maxc < 0) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "maxColumns must be >= 0"); return NULL; }
    const int64_t count = (int64_t)(slen / (size_t)S);
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0; double *ocnt = NULL, *ofirst = NULL;
    if (argc > 7 && !get_typed(env, argv[7], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 8 && !get_typed(env, argv[8], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 9 && !get_f64_out(env, argv[9], (size_t)S, &ocnt)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outCounts must be a Float64Array(S)"); return NULL; }
    if (argc > 10 && !get_f64_out(env, argv[10], (size_t)S, &ofirst)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outFirst must be a Float64Array(S)"); return NULL; }
    int32_t n_high, split;
    if (!get_multires_pair(env, argc, argv, 11, &n_high, &split)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "nHigh and splitRow must be integers"); return NULL; }
    BANDS_OR_THROW(13)
    const size_t cells = (size_t)S * (size_t)maxc * (size_t)h->rows;
    if ((db && dblen != cells) || (rgba && rgbalen != 4 * cells)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must hold S*maxColumns*rows floats, outRgba 4x that in bytes"); return NULL; }
    int64_t* tmp = (int64_t*)malloc((size_t)S * 2 * sizeof(int64_t));
    if (!tmp) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "malloc"); return NULL; }
    int rc = K > 0 ? emspec_push_samples_multiband(h->e, (const float*)smp, S, count, count, K, bn, bsplit, hop, reassign ? 1 : 0,
                                                   (float*)db, (uint8_t*)rgba, h->rows, maxc, tmp, tmp + S)
           : n_high > 0 ? emspec_push_samples_multires(h->e, (const float*)smp, S, count, count, n, n_high, hop, split, reassign ? 1 : 0,
                                                       (float*)db, (uint8_t*)rgba, h->rows, maxc, tmp, tmp + S)
                        : emspec_push_samples_multi(h->e, (const float*)smp, S, count, count, n, hop, reassign ? 1 : 0, (float*)db,
                                                    (uint8_t*)rgba, h->rows, maxc, tmp, tmp + S);
    if (rc == EMSPEC_OK) for (int32_t s = 0; s < S; ++s) { if (ocnt) ocnt[s] = (double)tmp[s]; if (ofirst) ofirst[s] = (double)tmp[S + s]; }
    free(tmp);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* ---- PCM front end (include/emspec.h: emspec_pcm_format; index.js: pcmFormat) ----
 * A format crosses as four arguments: sampleType (EMSPEC_PCM_*), channels, views, mix:Float32Array(views*channels).  They are
 * handed to the library as they are (it names the field that is wrong); the raw frames are a typed array whose element type
 * must be the format's: Int16Array (S16), Uint8Array (S24, three per sample), Int32Array (S32), Float32Array (F32). */
static int get_pcm_format(napi_env env, napi_value* argv, emspec_pcm_format* fmt) {
    memset(fmt, 0, sizeof(*fmt));
    void* mix = NULL; size_t mlen = 0;
    if (napi_get_value_int32(env, argv[0], &fmt->sample_type) != napi_ok || napi_get_value_int32(env, argv[1], &fmt->channels) != napi_ok ||
        napi_get_value_int32(env, argv[2], &fmt->views) != napi_ok || !get_typed(env, argv[3], napi_float32_array, &mix, &mlen, 0)) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "format: sampleType, channels, views must be integers and mix a Float32Array (use pcmFormat())");
        return 0;
    }
    const size_t cap = EMSPEC_PCM_MAX_VIEWS * EMSPEC_PCM_MAX_CHANNELS;
    if (fmt->channels >= 1 && fmt->channels <= EMSPEC_PCM_MAX_CHANNELS && fmt->views >= 1 && fmt->views <= EMSPEC_PCM_MAX_VIEWS &&
        mlen != (size_t)fmt->channels * (size_t)fmt->views) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "format.mix must hold views * channels weights");
        return 0;
    }
    memcpy(fmt->mix, mix, sizeof(float) * (mlen < cap ? mlen : cap));
    return 1;
}

/* the raw frames: data and byte length; throws EMSPEC_ERR_INVALID_ARG when the array's element type contradicts the format */
static int get_pcm_source(napi_env env, napi_value v, const emspec_pcm_format* fmt, void** data, size_t* bytes) {
    bool is = false;
    napi_typedarray_type ty; napi_value ab; size_t off, len;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is || napi_get_typedarray_info(env, v, &ty, &len, data, &ab, &off) != napi_ok) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "raw frames must be an Int16Array, Int32Array, Float32Array or Uint8Array (S24)");
        return 0;
    }
    napi_typedarray_type want; size_t esize;
    switch (fmt->sample_type) {
        case EMSPEC_PCM_S16: want = napi_int16_array; esize = 2; break;
        case EMSPEC_PCM_S24: want = napi_uint8_array; esize = 1; break;
        case EMSPEC_PCM_S32: want = napi_int32_array; esize = 4; break;
        case EMSPEC_PCM_F32: want = napi_float32_array; esize = 4; break;
        default: napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "format.sample_type is not one of EMSPEC_PCM_S16 / _S24 / _S32 / _F32"); return 0;
    }
    if (ty != want) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "the typed array's element type contradicts format.type (s16: Int16Array, s24: Uint8Array, s32: Int32Array, f32: Float32Array)");
        return 0;
    }
    *bytes = len * esize;
    return 1;
}

/* pcmFrameBytes(sampleType, channels, views, mix) -> bytes per frame, -1 for an invalid format (emspec_pcm_frame_bytes) */
static napi_value PcmFrameBytes(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcmFrameBytes(sampleType, channels, views, mix)"); return NULL; }
    emspec_pcm_format fmt;
    if (!get_pcm_format(env, argv, &fmt)) return NULL;
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_pcm_frame_bytes(&fmt), &r));
    return r;
}

/* (sources, frames) of a raw array: frames = bytes / (sources * frame bytes); 0 when the format is invalid (the library says why) */
static int pcm_frames(napi_env env, const emspec_pcm_format* fmt, int32_t sources, size_t bytes, int64_t* frames) {
    const int64_t fb = emspec_pcm_frame_bytes(fmt);
    *frames = 0;
    if (fb <= 0) return 1;
    if (sources < 1 || bytes % ((size_t)sources * (size_t)fb) != 0) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "the raw array must hold sources * frames whole frames");
        return 0;
    }
    *frames = (int64_t)(bytes / ((size_t)sources * (size_t)fb));
    return 1;
}

/* batchPcm(handle, src, sampleType, channels, views, mix, sources, fftSize, hop, reassign, outDb[, outRgba, outIndex]) -> columns.
 * emspec_batch_pcm: src holds sources * frames interleaved frames; outputs for sources * views streams. */
static napi_value BatchPcm(napi_env env, napi_callback_info info) {
    size_t argc = 13; napi_value argv[13];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 11) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchPcm(handle, src, sampleType, channels, views, mix, sources, fftSize, hop, reassign, outDb[, outRgba, outIndex])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    emspec_pcm_format fmt; void* src; size_t bytes;
    if (!get_pcm_format(env, argv + 2, &fmt) || !get_pcm_source(env, argv[1], &fmt, &src, &bytes)) return NULL;
    int32_t sources, n, hop; int64_t frames; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &sources));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[8], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[9], &argv[9]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[9], &reassign));
    if (!pcm_frames(env, &fmt, sources, bytes, &frames)) return NULL;
    size_t l0 = 0, l1 = 0, l2 = 0; void *p0 = NULL, *p1 = NULL, *p2 = NULL;
    if (!get_typed(env, argv[10], napi_float32_array, &p0, &l0, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 11 && !get_typed(env, argv[11], napi_uint8_array, &p1, &l1, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 12 && !get_typed(env, argv[12], napi_uint8_array, &p2, &l2, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array"); return NULL; }
    const int64_t C = frames > 0 ? out_columns(h, emspec_num_columns(frames, n, hop)) : 0;
    size_t cells = 0;
    if (p0) cells = l0; else if (p1) cells = l1 / 4; else if (p2) cells = l2;
    /* (C <= 0: an invalid format or shape - the library rejects it with its message before it touches any output) */
    if (C > 0 && (cells != (size_t)sources * (size_t)fmt.views * (size_t)C * (size_t)h->rows || (p1 && l1 != 4 * cells) || (p2 && l2 != cells) || (p0 && l0 != cells))) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "output arrays must hold exactly sources*views*columns*rows cells, rows = the engine's row count (rgba: 4 bytes per cell)");
        return NULL;
    }
    emspec_out out; memset(&out, 0, sizeof(out));
    out.db = (float*)p0; out.rgba = (uint8_t*)p1; out.index = (uint8_t*)p2;
    int rc = emspec_batch_pcm(h->e, src, &fmt, sources, frames, n, hop, reassign ? 1 : 0, &out);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}

/* batchPcmPacked(handle, src, sampleType, channels, views, mix, sources, fftSize, hop, reassign, wire, offsets:Float64Array(sources*views+1)) -> columns */
static napi_value BatchPcmPacked(napi_env env, napi_callback_info info) {
    size_t argc = 12; napi_value argv[12];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 12) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchPcmPacked(handle, src, sampleType, channels, views, mix, sources, fftSize, hop, reassign, wire, offsets)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    emspec_pcm_format fmt; void* src; size_t bytes;
    if (!get_pcm_format(env, argv + 2, &fmt) || !get_pcm_source(env, argv[1], &fmt, &src, &bytes)) return NULL;
    int32_t sources, n, hop; int64_t frames; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &sources));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[8], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[9], &argv[9]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[9], &reassign));
    if (!pcm_frames(env, &fmt, sources, bytes, &frames)) return NULL;
    void *wire = NULL, *offs = NULL; size_t wlen = 0, olen = 0;
    if (!get_typed(env, argv[10], napi_uint8_array, &wire, &wlen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "wire must be a Uint8Array"); return NULL; }
    const size_t S = frames > 0 ? (size_t)sources * (size_t)fmt.views : 0;
    if (!get_typed(env, argv[11], napi_float64_array, &offs, &olen, 0) || (S && olen != S + 1)) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "offsets must be a Float64Array(sources * views + 1)"); return NULL;
    }
    int64_t* o64 = (int64_t*)malloc(sizeof(int64_t) * (S + 1));
    if (!o64) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "out of host memory"); return NULL; }
    int rc = emspec_batch_pcm_packed(h->e, src, &fmt, sources, frames, n, hop, reassign ? 1 : 0, (uint8_t*)wire, (int64_t)wlen, o64);
    if (rc == EMSPEC_OK) for (size_t i = 0; i <= S; ++i) ((double*)offs)[i] = (double)o64[i];
    free(o64);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, out_columns(h, emspec_num_columns(frames, n, hop)), &r));
    return r;
}

/* pushPcm(handle, block, sampleType, channels, views, mix, sources, fftSize, hop, reassign, maxColumns, outDb?, outRgba?,
 *         outCounts?:Float64Array(sources*views), outFirst?[, nHigh, splitRow[, fftSizes, splitRows]]): emspec_push_samples_pcm /
 *         _pcm_multires / _pcm_multiband; block holds
 *         `count` frames of every source, source after source. */
static napi_value PushPcm(napi_env env, napi_callback_info info) {
    size_t argc = 19; napi_value argv[19];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 11) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pushPcm(handle, block, sampleType, channels, views, mix, sources, fftSize, hop, reassign, maxColumns[, outDb, outRgba, outCounts, outFirst, nHigh, splitRow])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    emspec_pcm_format fmt; void* blk; size_t bytes;
    if (!get_pcm_format(env, argv + 2, &fmt) || !get_pcm_source(env, argv[1], &fmt, &blk, &bytes)) return NULL;
    int32_t sources, n, hop; int64_t maxc, count; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &sources));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[8], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[9], &argv[9]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[9], &reassign));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[10], &maxc));
    if (!pcm_frames(env, &fmt, sources, bytes, &count)) return NULL;
    if (maxc < 0) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "maxColumns must be >= 0"); return NULL; }
    const int64_t fb = emspec_pcm_frame_bytes(&fmt);
    const size_t S = fb > 0 ? (size_t)sources * (size_t)fmt.views : 1;
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0; double *ocnt = NULL, *ofirst = NULL;
    if (argc > 11 && !get_typed(env, argv[11], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 12 && !get_typed(env, argv[12], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 13 && !get_f64_out(env, argv[13], S, &ocnt)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outCounts must be a Float64Array(sources * views)"); return NULL; }
    if (argc > 14 && !get_f64_out(env, argv[14], S, &ofirst)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outFirst must be a Float64Array(sources * views)"); return NULL; }
    int32_t n_high, split;
    if (!get_multires_pair(env, argc, argv, 15, &n_high, &split)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "nHigh and splitRow must be integers"); return NULL; }
    BANDS_OR_THROW(17)
    const size_t cells = S * (size_t)maxc * (size_t)h->rows;
    if (fb > 0 && ((db && dblen != cells) || (rgba && rgbalen != 4 * cells))) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must hold sources*views*maxColumns*rows floats, outRgba 4x that in bytes"); return NULL; }
    int64_t* tmp = (int64_t*)malloc(S * 2 * sizeof(int64_t));
    if (!tmp) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "malloc"); return NULL; }
    const int64_t stride = count * (fb > 0 ? fb : 0);
    int rc = K > 0 ? emspec_push_samples_pcm_multiband(h->e, blk, &fmt, sources, count, stride, K, bn, bsplit, hop, reassign ? 1 : 0,
                                                       (float*)db, (uint8_t*)rgba, h->rows, maxc, tmp, tmp + S)
           : n_high > 0 ? emspec_push_samples_pcm_multires(h->e, blk, &fmt, sources, count, stride, n, n_high, hop, split, reassign ? 1 : 0,
                                                           (float*)db, (uint8_t*)rgba, h->rows, maxc, tmp, tmp + S)
                        : emspec_push_samples_pcm(h->e, blk, &fmt, sources, count, stride, n, hop, reassign ? 1 : 0, (float*)db,
                                                  (uint8_t*)rgba, h->rows, maxc, tmp, tmp + S);
    if (rc == EMSPEC_OK) for (size_t s = 0; s < S; ++s) { if (ocnt) ocnt[s] = (double)tmp[s]; if (ofirst) ofirst[s] = (double)tmp[S + s]; }
    free(tmp);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

static napi_value ResetStream(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "resetStream(handle, stream)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t s;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &s));
    int rc = emspec_reset_stream(h->e, s);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

static napi_value LiveStreams(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int32(env, emspec_live_streams(h->e), &r));
    return r;
}

/* columnsAsync(handle, frames, S, fftSize, hop, reassign, outDb?, outRgba?, outColumns?) -> Promise<undefined>: columns() on the
 * libuv thread pool (napi_create_async_work).  The typed arrays are kept alive by references; the caller touches neither them
 * nor the engine before the promise settles (an engine is not thread-safe). */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[4];
    emspec_engine* e;
    const float* frames;
    float* db; uint8_t* rgba; double* ocol; int64_t* c64;
    int32_t S, n, hop, reassign, rows;
    int rc;
    char msg[256];
} columns_job;

static void columns_execute(napi_env env, void* data) {
    (void)env;
    columns_job* j = (columns_job*)data;
    j->rc = emspec_columns(j->e, j->frames, j->S, j->n, j->hop, j->reassign, j->db, j->rgba, j->rows, j->c64);
    if (j->rc != EMSPEC_OK) { strncpy(j->msg, emspec_last_error(j->e), sizeof(j->msg) - 1); j->msg[sizeof(j->msg) - 1] = 0; }
}

static void columns_complete(napi_env env, napi_status status, void* data) {
    columns_job* j = (columns_job*)data;
    if (status == napi_ok && j->rc == EMSPEC_OK) {
        if (j->ocol) for (int32_t s = 0; s < j->S; ++s) j->ocol[s] = (double)j->c64[s];
        napi_value v; napi_get_undefined(env, &v);
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value code, msg, err;
        napi_create_string_utf8(env, status == napi_ok ? status_name(j->rc) : "EMSPEC_NAPI", NAPI_AUTO_LENGTH, &code);
        napi_create_string_utf8(env, status == napi_ok ? j->msg : "async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, code, msg, &err);
        napi_reject_deferred(env, j->deferred, err);
    }
    for (int i = 0; i < 4; ++i) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
    napi_delete_async_work(env, j->work);
    free(j->c64);
    free(j);
}

static napi_value ColumnsAsync(napi_env env, napi_callback_info info) {
    size_t argc = 9; napi_value argv[9];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 6) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "columnsAsync(handle, frames, S, fftSize, hop, reassign[, outDb, outRgba, outColumns])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* fr; size_t flen;
    if (!get_typed(env, argv[1], napi_float32_array, &fr, &flen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "frames must be a Float32Array"); return NULL; }
    int32_t S, n, hop; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[5], &argv[5]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[5], &reassign));
    if (S < 1 || n < 1 || (size_t)S * (size_t)n != flen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "frames.length must equal S*fftSize"); return NULL; }
    void *db = NULL, *rgba = NULL; size_t dblen = 0, rgbalen = 0; double* ocol = NULL;
    if (argc > 6 && !get_typed(env, argv[6], napi_float32_array, &db, &dblen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    if (argc > 7 && !get_typed(env, argv[7], napi_uint8_array, &rgba, &rgbalen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array"); return NULL; }
    if (argc > 8 && !get_f64_out(env, argv[8], (size_t)S, &ocol)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outColumns must be a Float64Array(S)"); return NULL; }
    const size_t cells = (size_t)S * (size_t)h->rows;
    if ((db && dblen != cells) || (rgba && rgbalen != 4 * cells)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must hold S*rows floats, outRgba 4*S*rows bytes (rows = the engine's row count)"); return NULL; }
    columns_job* j = (columns_job*)calloc(1, sizeof(columns_job));
    if (!j) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "calloc"); return NULL; }
    j->c64 = (int64_t*)malloc((size_t)S * sizeof(int64_t));
    if (!j->c64) { free(j); napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "malloc"); return NULL; }
    j->e = h->e; j->frames = (const float*)fr; j->db = (float*)db; j->rgba = (uint8_t*)rgba; j->ocol = ocol;
    j->S = S; j->n = n; j->hop = hop; j->reassign = reassign ? 1 : 0; j->rows = h->rows;
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) { free(j->c64); free(j); napi_throw_error(env, "EMSPEC_NAPI", "napi_create_promise"); return NULL; }
    napi_create_reference(env, argv[1], 1, &j->refs[0]);
    if (db) napi_create_reference(env, argv[6], 1, &j->refs[1]);
    if (rgba) napi_create_reference(env, argv[7], 1, &j->refs[2]);
    if (ocol) napi_create_reference(env, argv[8], 1, &j->refs[3]);
    napi_create_string_utf8(env, "emspec.columnsAsync", NAPI_AUTO_LENGTH, &name);
    if (napi_create_async_work(env, NULL, name, columns_execute, columns_complete, j, &j->work) != napi_ok ||
        napi_queue_async_work(env, j->work) != napi_ok) {
        for (int i = 0; i < 4; ++i) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
        free(j->c64); free(j);
        napi_throw_error(env, "EMSPEC_NAPI", "could not queue async work");
        return NULL;
    }
    return promise;
}

static napi_value SetColormap(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* lut; size_t len;
    if (argc < 2 || !get_typed(env, argv[1], napi_uint8_array, &lut, &len, 0) || len != 1024) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "colormap must be a Uint8Array(1024) of RGBA"); return NULL; }
    int rc = emspec_set_colormap(h->e, (const uint8_t*)lut);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

static napi_value SetDisplay(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    double sm = 0, agc = 0;
    if (argc < 3 || napi_get_value_double(env, argv[1], &sm) != napi_ok || napi_get_value_double(env, argv[2], &agc) != napi_ok) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setDisplay(handle, smoothing, agcStrength)"); return NULL; }
    int rc = emspec_set_display(h->e, (float)sm, (float)agc);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* setTimeReduce(handle, factor): emspec_set_time_reduce (1 = off .. 65536); timeReduce(handle) -> the factor in force;
 * reducedColumns(columns, factor) -> ceil(columns / factor), -1 on invalid arguments (no engine) */
static napi_value SetTimeReduce(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t f = 0;
    if (argc < 2 || napi_get_value_int32(env, argv[1], &f) != napi_ok) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setTimeReduce(handle, factor)"); return NULL; }
    int rc = emspec_set_time_reduce(h->e, f);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
static napi_value TimeReduce(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int32(env, emspec_time_reduce(h->e), &r));
    return r;
}
static napi_value ReducedColumns(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int64_t c = 0; int32_t f = 0;
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "reducedColumns(columns, factor)"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[0], &c));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &f));
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_reduced_columns(c, f), &r));
    return r;
}

/* setRowEdges(handle, Float32Array(rows+1) | null) ; getRowEdges(handle, Float32Array(rows+1)) */
static napi_value SetRowEdges(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* p = NULL; size_t len = 0;
    if (argc < 2 || !get_typed(env, argv[1], napi_float32_array, &p, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "edges must be a Float32Array(rows+1) or null"); return NULL; }
    int rc = emspec_set_row_edges_hz(h->e, (const float*)p, (int32_t)len);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
static napi_value GetRowEdges(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* p = NULL; size_t len = 0;
    if (argc < 2 || !get_typed(env, argv[1], napi_float32_array, &p, &len, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "out must be a Float32Array(rows+1)"); return NULL; }
    int rc = emspec_get_row_edges_hz(h->e, (float*)p, (int32_t)len);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* Spectral peaks (include/emspec.h).
 * batchPeaks(handle, pcm:Float32Array(S*L), S, L, fftSize, hop, reassign, k, minDb, out:Float32Array(S*C*k*2)) -> columns per
 *   stream: emspec_batch_peaks - only the peak lists cross PCIe on the way out
 * peaksOf(db:Float32Array(columns*rows), columns, rows, k, minDb, out:Float32Array(columns*k*2)): emspec_peaks_host (no device,
 *   no engine)
 * positionHz(handle, pos) -> Hz: emspec_position_hz */
static napi_value BatchPeaks(napi_env env, napi_callback_info info) {
    size_t argc = 10; napi_value argv[10];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 10) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchPeaks(handle, pcm, S, L, fftSize, hop, reassign, k, minDb, out)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void *pcm = NULL, *out = NULL; size_t plen = 0, olen = 0;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S = 0, n = 0, hop = 0, k = 0; int64_t L = 0; bool reassign = true; double min_db = 0.0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &hop));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[6], &reassign));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &k));
    NAPI_OK_OR_RETURN(env, napi_get_value_double(env, argv[8], &min_db));
    if (!get_typed(env, argv[9], napi_float32_array, &out, &olen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "out must be a Float32Array"); return NULL; }
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    const int64_t C = emspec_num_columns(L, n, hop);
    /* (C <= 0 or k outside 1..32: the library rejects the call with its message before it touches the output) */
    if (C > 0 && k >= 1 && k <= 32 && olen != (size_t)S * (size_t)C * (size_t)k * 2) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "out must hold exactly S*columns*k*2 floats");
        return NULL;
    }
    int rc = emspec_batch_peaks(h->e, (const float*)pcm, S, L, n, hop, reassign ? 1 : 0, k, (float)min_db, (emspec_peak*)out);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}
static napi_value PeaksOf(napi_env env, napi_callback_info info) {
    size_t argc = 6; napi_value argv[6];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 6) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "peaksOf(db, columns, rows, k, minDb, out)"); return NULL; }
    void *db = NULL, *out = NULL; size_t dlen = 0, olen = 0;
    if (!get_typed(env, argv[0], napi_float32_array, &db, &dlen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "db must be a Float32Array"); return NULL; }
    int64_t columns = 0; int32_t rows = 0, k = 0; double min_db = 0.0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &columns));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &rows));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &k));
    NAPI_OK_OR_RETURN(env, napi_get_value_double(env, argv[4], &min_db));
    if (!get_typed(env, argv[5], napi_float32_array, &out, &olen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "out must be a Float32Array"); return NULL; }
    if (columns >= 0 && rows >= 4 && k >= 1 && k <= 32 &&
        (dlen != (size_t)columns * (size_t)rows || olen != (size_t)columns * (size_t)k * 2)) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "db must hold columns*rows floats and out columns*k*2");
        return NULL;
    }
    int rc = emspec_peaks_host((const float*)db, columns, rows, k, (float)min_db, (emspec_peak*)out);
    if (rc != EMSPEC_OK) return throw_status(env, NULL, rc);
    return NULL;
}
/* Waveform envelope (include/emspec.h).
 * setWaveOut(handle, wave:Float32Array | null): emspec_set_wave_out with capacity wave.length / 2 pairs - while set, the batch
 *   calls that run the host pipeline also fill it; the addon references the array until it is replaced, cleared or the engine
 *   is destroyed
 * waveOf(pcm:Float32Array(S*L), S, L, fftSize, hop, factor, out:Float32Array(S*Cr*2)): emspec_wave_host (no device, no engine) */
static napi_value SetWaveOut(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setWaveOut(handle, wave)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* wave = NULL; size_t wlen = 0;
    if (!get_typed(env, argv[1], napi_float32_array, &wave, &wlen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "wave must be a Float32Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (wave) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[1], 1, &ref));
    int rc = emspec_set_wave_out(h->e, (emspec_wave*)wave, wave ? (int64_t)(wlen / 2) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_wave(env, h);
    h->wave = ref;
    return NULL;
}
/* Level meters (include/emspec.h).  Records travel as bytes: index.js lays BigUint64Array / BigInt64Array
 * views over them.
 * setLevelOut(handle, level:Uint8Array | null): emspec_set_level_out with capacity level.length / 24 records
 * setCrossOut(handle, a, b, cross:Uint8Array | null): emspec_set_cross_out with capacity cross.length / 16 records
 *   While set, the batch calls that run the host pipeline also fill them; the addon references an array until it is replaced,
 *   cleared or the engine is destroyed.
 * levelsOf(pcm:Float32Array(S*L), S, L, fftSize, hop, factor, out:Uint8Array(S*Cr*24)): emspec_level_host
 * crossOf(pcm, pairs, views, a, b, L, fftSize, hop, factor, out:Uint8Array(pairs*Cr*16)): emspec_cross_host
 * levelWindow(L, fftSize, hop, factor, g) -> samples;  levelValues(level:Uint8Array(24), samples) -> [rmsDb, peakDb];
 * crossCorrelation(a:Uint8Array(24), b:Uint8Array(24), ab:Uint8Array(16)) -> rho */
static napi_value SetLevelOut(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLevelOut(handle, level)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* arr = NULL; size_t len = 0;
    if (!get_typed(env, argv[1], napi_uint8_array, &arr, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "level must be a Uint8Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (arr) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[1], 1, &ref));
    int rc = emspec_set_level_out(h->e, (emspec_level*)arr, arr ? (int64_t)(len / sizeof(emspec_level)) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_ref(env, &h->level);
    h->level = ref;
    return NULL;
}
static napi_value SetCrossOut(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setCrossOut(handle, a, b, cross)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t a = 0, b = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &a));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &b));
    void* arr = NULL; size_t len = 0;
    if (!get_typed(env, argv[3], napi_uint8_array, &arr, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "cross must be a Uint8Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (arr) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[3], 1, &ref));
    int rc = emspec_set_cross_out(h->e, a, b, (emspec_cross*)arr, arr ? (int64_t)(len / sizeof(emspec_cross)) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_ref(env, &h->cross);
    h->cross = ref;
    return NULL;
}
/* the shared tail of levelsOf / crossOf: argv[at ..] = L, fftSize, hop, factor, out; rows records of `size` bytes per delivered column */
static int level_shape(napi_env env, napi_value* argv, int at, int64_t rows, size_t size, int64_t* L, int32_t* n, int32_t* hop, int32_t* factor,
                       void** out) {
    size_t olen = 0;
    if (napi_get_value_int64(env, argv[at], L) != napi_ok || napi_get_value_int32(env, argv[at + 1], n) != napi_ok ||
        napi_get_value_int32(env, argv[at + 2], hop) != napi_ok || napi_get_value_int32(env, argv[at + 3], factor) != napi_ok) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "L, fftSize, hop and factor must be numbers");
        return 0;
    }
    if (!get_typed(env, argv[at + 4], napi_uint8_array, out, &olen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "out must be a Uint8Array"); return 0; }
    /* (a shape the library rejects: it does so with its message before it touches the output) */
    const int64_t C = emspec_num_columns(*L, *n, *hop), Cr = C >= 0 ? emspec_reduced_columns(C, *factor) : -1;
    if (Cr >= 0 && rows >= 0 && olen != (size_t)rows * (size_t)Cr * size) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "out must hold exactly rows*reducedColumns records");
        return 0;
    }
    return 1;
}
static napi_value LevelsOf(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 7) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "levelsOf(pcm, S, L, fftSize, hop, factor, out)"); return NULL; }
    void *pcm = NULL, *out = NULL; size_t plen = 0;
    if (!get_typed(env, argv[0], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S = 0, n = 0, hop = 0, factor = 0; int64_t L = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &S));
    if (!level_shape(env, argv, 2, S, sizeof(emspec_level), &L, &n, &hop, &factor, &out)) return NULL;
    if (S < 0 || L < 0 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    int rc = emspec_level_host((const float*)pcm, S, L, n, hop, factor, (emspec_level*)out);
    if (rc != EMSPEC_OK) return throw_status(env, NULL, rc);
    return NULL;
}
static napi_value CrossOf(napi_env env, napi_callback_info info) {
    size_t argc = 10; napi_value argv[10];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 10) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "crossOf(pcm, pairs, views, a, b, L, fftSize, hop, factor, out)"); return NULL; }
    void *pcm = NULL, *out = NULL; size_t plen = 0;
    if (!get_typed(env, argv[0], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t pairs = 0, views = 0, a = 0, b = 0, n = 0, hop = 0, factor = 0; int64_t L = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &pairs));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &views));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &a));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &b));
    if (!level_shape(env, argv, 5, pairs, sizeof(emspec_cross), &L, &n, &hop, &factor, &out)) return NULL;
    if (pairs < 0 || views < 0 || L < 0 || (size_t)pairs * (size_t)views * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal pairs*views*L"); return NULL; }
    int rc = emspec_cross_host((const float*)pcm, pairs, views, a, b, L, n, hop, factor, (emspec_cross*)out);
    if (rc != EMSPEC_OK) return throw_status(env, NULL, rc);
    return NULL;
}
static napi_value LevelWindow(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "levelWindow(L, fftSize, hop, factor, g)"); return NULL; }
    int64_t L = 0, g = 0; int32_t n = 0, hop = 0, factor = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[0], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &hop));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &factor));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[4], &g));
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_level_window(L, n, hop, factor, g), &r));
    return r;
}
/* one record of `size` bytes out of a Uint8Array (copied: a view may lie at any byte offset) */
static int get_record(napi_env env, napi_value v, void* rec, size_t size) {
    void* p = NULL; size_t len = 0;
    if (!get_typed(env, v, napi_uint8_array, &p, &len, 0) || len != size) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "a record must be a Uint8Array of its size (24 or 16 bytes)");
        return 0;
    }
    memcpy(rec, p, size);
    return 1;
}
static napi_value LevelValues(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "levelValues(level, samples)"); return NULL; }
    emspec_level lv; int64_t samples = 0; double rms = 0.0, peak = 0.0;
    if (!get_record(env, argv[0], &lv, sizeof lv)) return NULL;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &samples));
    if (emspec_level_values(&lv, samples, &rms, &peak) != EMSPEC_OK) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "levelValues needs samples >= 1"); return NULL; }
    napi_value r, a, b;
    NAPI_OK_OR_RETURN(env, napi_create_array_with_length(env, 2, &r));
    NAPI_OK_OR_RETURN(env, napi_create_double(env, rms, &a));
    NAPI_OK_OR_RETURN(env, napi_create_double(env, peak, &b));
    NAPI_OK_OR_RETURN(env, napi_set_element(env, r, 0, a));
    NAPI_OK_OR_RETURN(env, napi_set_element(env, r, 1, b));
    return r;
}
static napi_value CrossCorrelation(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "crossCorrelation(levelA, levelB, cross)"); return NULL; }
    emspec_level a, b; emspec_cross ab; double rho = 0.0;
    if (!get_record(env, argv[0], &a, sizeof a) || !get_record(env, argv[1], &b, sizeof b) || !get_record(env, argv[2], &ab, sizeof ab)) return NULL;
    if (emspec_cross_correlation(&a, &b, &ab, &rho) != EMSPEC_OK) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "crossCorrelation"); return NULL; }
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_double(env, rho, &r));
    return r;
}
/* Overlays of the live calls (include/emspec.h: emspec_set_live_peaks / emspec_set_live_wave).
 * setLivePeaks(handle, k, minDb, peaks:Float32Array | null): capacity peaks.length / 2 pairs
 * setLiveWave(handle, wave:Float32Array | null): capacity wave.length / 2 pairs
 * While set, every live call also fills them; the addon references an array until it is replaced, cleared or the engine is
 * destroyed.  index.js hands over page-locked arrays, which the kernel writes in place. */
static napi_value SetLivePeaks(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLivePeaks(handle, k, minDb, peaks)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t k = 0; double min_db = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &k));
    NAPI_OK_OR_RETURN(env, napi_get_value_double(env, argv[2], &min_db));
    void* arr = NULL; size_t len = 0;
    if (!get_typed(env, argv[3], napi_float32_array, &arr, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "peaks must be a Float32Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (arr) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[3], 1, &ref));
    int rc = emspec_set_live_peaks(h->e, k, (float)min_db, (emspec_peak*)arr, arr ? (int64_t)(len / 2) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_ref(env, &h->live_peaks);
    h->live_peaks = ref;
    return NULL;
}
static napi_value SetLiveWave(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLiveWave(handle, wave)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* arr = NULL; size_t len = 0;
    if (!get_typed(env, argv[1], napi_float32_array, &arr, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "wave must be a Float32Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (arr) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[1], 1, &ref));
    int rc = emspec_set_live_wave(h->e, (emspec_wave*)arr, arr ? (int64_t)(len / 2) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_ref(env, &h->live_wave);
    h->live_wave = ref;
    return NULL;
}
/* Live level meters (include/emspec.h: emspec_set_live_level / emspec_set_live_cross / emspec_level_sum / emspec_cross_sum).
 * setLiveLevel(handle, level:Uint8Array | null): capacity level.length / 24 records
 * setLiveCross(handle, views, a, b, cross:Uint8Array | null): capacity cross.length / 16 records
 * levelSum(records:Uint8Array(count*24), out:Uint8Array(24));  crossSum(records:Uint8Array(count*16), out:Uint8Array(16))
 * The arrays are referenced as the other overlays' are. */
static napi_value SetLiveLevel(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLiveLevel(handle, level)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* arr = NULL; size_t len = 0;
    if (!get_typed(env, argv[1], napi_uint8_array, &arr, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "level must be a Uint8Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (arr) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[1], 1, &ref));
    int rc = emspec_set_live_level(h->e, (emspec_level*)arr, arr ? (int64_t)(len / sizeof(emspec_level)) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_ref(env, &h->live_level);
    h->live_level = ref;
    return NULL;
}
static napi_value SetLiveCross(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLiveCross(handle, views, a, b, cross)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t views = 0, a = 0, b = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &views));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &a));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &b));
    void* arr = NULL; size_t len = 0;
    if (!get_typed(env, argv[4], napi_uint8_array, &arr, &len, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "cross must be a Uint8Array or null"); return NULL; }
    napi_ref ref = NULL;
    if (arr) NAPI_OK_OR_RETURN(env, napi_create_reference(env, argv[4], 1, &ref));
    int rc = emspec_set_live_cross(h->e, views, a, b, (emspec_cross*)arr, arr ? (int64_t)(len / sizeof(emspec_cross)) : 0);
    if (rc != EMSPEC_OK) {
        if (ref) napi_delete_reference(env, ref);
        return throw_status(env, h->e, rc);
    }
    drop_ref(env, &h->live_cross);
    h->live_cross = ref;
    return NULL;
}
/* the shared body of levelSum / crossSum: records of `size` bytes, copied (a view may lie at any byte offset) */
static napi_value records_sum(napi_env env, napi_callback_info info, size_t size, const char* usage) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    void *rec = NULL, *out = NULL; size_t rlen = 0, olen = 0;
    if (argc < 2 || !get_typed(env, argv[0], napi_uint8_array, &rec, &rlen, 0) || !get_typed(env, argv[1], napi_uint8_array, &out, &olen, 0) ||
        olen != size || rlen % size) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", usage);
        return NULL;
    }
    const int64_t count = (int64_t)(rlen / size);
    void* copy = malloc(rlen ? rlen : 1);
    if (!copy) { napi_throw_error(env, "EMSPEC_ERR_OUT_OF_MEMORY", "out of memory"); return NULL; }
    memcpy(copy, rec, rlen);
    emspec_level lsum; emspec_cross xsum;
    const int rc = size == sizeof(emspec_level) ? emspec_level_sum((const emspec_level*)copy, count, &lsum)
                                                : emspec_cross_sum((const emspec_cross*)copy, count, &xsum);
    free(copy);
    if (rc != EMSPEC_OK) return throw_status(env, NULL, rc);
    memcpy(out, size == sizeof(emspec_level) ? (const void*)&lsum : (const void*)&xsum, size);
    return NULL;
}
static napi_value LevelSum(napi_env env, napi_callback_info info) {
    return records_sum(env, info, sizeof(emspec_level), "levelSum(records:Uint8Array(count*24), out:Uint8Array(24))");
}
static napi_value CrossSum(napi_env env, napi_callback_info info) {
    return records_sum(env, info, sizeof(emspec_cross), "crossSum(records:Uint8Array(count*16), out:Uint8Array(16))");
}
/* Live history (include/emspec.h: emspec_set_live_history / emspec_live_history / emspec_history_view).
 * setLiveHistory(handle, columns): W columns per stream, 0 clears
 * liveHistory(handle, session, stream) -> [end, first] or null (no history, or the session has no such stream)
 * historyView(handle, session, stream0, streams, firstColumn, factor, groups, map:Float32Array(4) | null,
 *             outDb:Float32Array | null, outIndex:Uint8Array | null, outRgba:Uint8Array | null): the arrays hold exactly
 *             streams * groups * rows cells (RGBA: x 4); map = [dbTop, dbRange, gateDb, shiftDb] */
static napi_value SetLiveHistory(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLiveHistory(handle, columns)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int64_t w = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &w));
    int rc = emspec_set_live_history(h->e, w);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
static napi_value LiveHistory(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "liveHistory(handle, session, stream)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t session = 0, stream = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &session));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &stream));
    int64_t first = -1;
    const int64_t end = emspec_live_history(h->e, session, stream, &first);
    napi_value r;
    if (end < 0) { NAPI_OK_OR_RETURN(env, napi_get_null(env, &r)); return r; }
    napi_value a, b;
    NAPI_OK_OR_RETURN(env, napi_create_array_with_length(env, 2, &r));
    NAPI_OK_OR_RETURN(env, napi_create_int64(env, end, &a));
    NAPI_OK_OR_RETURN(env, napi_create_int64(env, first, &b));
    NAPI_OK_OR_RETURN(env, napi_set_element(env, r, 0, a));
    NAPI_OK_OR_RETURN(env, napi_set_element(env, r, 1, b));
    return r;
}
static napi_value HistoryView(napi_env env, napi_callback_info info) {
    size_t argc = 11; napi_value argv[11];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 11) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "historyView(handle, session, stream0, streams, firstColumn, factor, groups, map, outDb, outIndex, outRgba)");
        return NULL;
    }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t session = 0, stream0 = 0, streams = 0, factor = 0; int64_t first = 0, groups = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &session));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &stream0));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &streams));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[4], &first));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &factor));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[6], &groups));
    void *mp = NULL, *db = NULL, *idx = NULL, *rgba = NULL; size_t mlen = 0, dlen = 0, ilen = 0, rlen = 0;
    if (!get_typed(env, argv[7], napi_float32_array, &mp, &mlen, 1) || (mp && mlen != 4)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "map must be a Float32Array(4) or null"); return NULL; }
    if (!get_typed(env, argv[8], napi_float32_array, &db, &dlen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array or null"); return NULL; }
    if (!get_typed(env, argv[9], napi_uint8_array, &idx, &ilen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array or null"); return NULL; }
    if (!get_typed(env, argv[10], napi_uint8_array, &rgba, &rlen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array or null"); return NULL; }
    /* (streams or groups below 1: the library rejects the call with its message before it touches an output) */
    if (streams >= 1 && groups >= 1) {
        const size_t cells = (size_t)streams * (size_t)groups * (size_t)h->rows;
        if ((db && dlen != cells) || (idx && ilen != cells) || (rgba && rlen != 4 * cells)) {
            napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "every output must hold exactly streams*groups*rows cells (RGBA: x 4)");
            return NULL;
        }
    }
    emspec_view_map m;
    if (mp) { const float* f = (const float*)mp; m.db_top = f[0]; m.db_range = f[1]; m.gate_db = f[2]; m.shift_db = f[3]; }
    int rc = emspec_history_view(h->e, session, stream0, streams, first, factor, groups, mp ? &m : NULL, (float*)db, (uint8_t*)idx, (uint8_t*)rgba);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* Stereo image (include/emspec.h: emspec_make_stereo_colormap / emspec_set_stereo_colormap / emspec_batch_pcm_stereo /
 * emspec_history_view_stereo).  map = Float32Array(5) [dbTop, dbRange, gateDb, shiftDb, panRangeDb] or null (the engine's
 * configuration, shift 0, 12 dB to a side); outputs: level Float32Array, index / pan Uint8Array, rgba Uint8Array (x 4), each of
 * exactly pairs * columns (groups) * rows cells or null.
 * stereoColormap(brightness) -> Uint8Array(33 * 1024)
 * setStereoColormap(handle, palette:Uint8Array(33 * 1024))
 * batchPcmStereo(handle, src, sampleType, channels, views, mix, sources, fftSize, hop, reassign, a, b, map, outLevel, outIndex,
 *                outPan, outRgba) -> columns
 * historyViewStereo(handle, session, stream0, pairs, views, a, b, firstColumn, factor, groups, map, outLevel, outIndex, outPan,
 *                   outRgba) */
static int get_stereo_map(napi_env env, napi_value v, emspec_stereo_map* m, int* have) {
    void* mp = NULL; size_t mlen = 0;
    if (!get_typed(env, v, napi_float32_array, &mp, &mlen, 1) || (mp && mlen != 5)) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "map must be a Float32Array(5) or null");
        return 0;
    }
    *have = mp != NULL;
    if (mp) { const float* f = (const float*)mp; m->db_top = f[0]; m->db_range = f[1]; m->gate_db = f[2]; m->shift_db = f[3]; m->pan_range_db = f[4]; }
    return 1;
}
/* the four outputs from argv[0 .. 3]; *cells: what the first one given holds (0: none) */
static int get_stereo_outs(napi_env env, const napi_value* argv, void** out, size_t* len) {
    static const napi_typedarray_type ty[4] = {napi_float32_array, napi_uint8_array, napi_uint8_array, napi_uint8_array};
    static const char* const what[4] = {"outLevel must be a Float32Array or null", "outIndex must be a Uint8Array or null",
                                        "outPan must be a Uint8Array or null", "outRgba must be a Uint8Array or null"};
    for (int i = 0; i < 4; ++i) {
        out[i] = NULL; len[i] = 0;
        if (!get_typed(env, argv[i], ty[i], &out[i], &len[i], 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", what[i]); return 0; }
    }
    return 1;
}
static int stereo_outs_hold(napi_env env, void* const* out, const size_t* len, size_t cells) {
    for (int i = 0; i < 4; ++i)
        if (out[i] && len[i] != (i == 3 ? 4 * cells : cells)) {
            napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "every output must hold exactly pairs*columns*rows cells (RGBA: x 4)");
            return 0;
        }
    return 1;
}
static napi_value StereoColormap(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    double b = 0.5;
    if (argc > 0) NAPI_OK_OR_RETURN(env, napi_get_value_double(env, argv[0], &b));
    napi_value ab, out; void* data;
    const size_t bytes = (size_t)EMSPEC_STEREO_PAN_LEVELS * 1024;
    NAPI_OK_OR_RETURN(env, napi_create_arraybuffer(env, bytes, &data, &ab));
    if (emspec_make_stereo_colormap((float)b, (uint8_t*)data) != EMSPEC_OK) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "brightness must be >= 0"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &out));
    return out;
}
static napi_value SetStereoColormap(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pal; size_t len;
    if (argc < 2 || !get_typed(env, argv[1], napi_uint8_array, &pal, &len, 0) || len != (size_t)EMSPEC_STEREO_PAN_LEVELS * 1024) {
        napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "the stereo palette must be a Uint8Array(33 * 1024) of RGBA");
        return NULL;
    }
    int rc = emspec_set_stereo_colormap(h->e, (const uint8_t*)pal);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
static napi_value BatchPcmStereo(napi_env env, napi_callback_info info) {
    size_t argc = 17; napi_value argv[17];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 17) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchPcmStereo(handle, src, sampleType, channels, views, mix, sources, fftSize, hop, reassign, a, b, map, outLevel, outIndex, outPan, outRgba)");
        return NULL;
    }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    emspec_pcm_format fmt; void* src; size_t bytes;
    if (!get_pcm_format(env, argv + 2, &fmt) || !get_pcm_source(env, argv[1], &fmt, &src, &bytes)) return NULL;
    int32_t sources, n, hop, a, b; int64_t frames; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &sources));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[8], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[9], &argv[9]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[9], &reassign));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[10], &a));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[11], &b));
    if (!pcm_frames(env, &fmt, sources, bytes, &frames)) return NULL;
    emspec_stereo_map m; int have = 0;
    if (!get_stereo_map(env, argv[12], &m, &have)) return NULL;
    void* out[4]; size_t len[4];
    if (!get_stereo_outs(env, argv + 13, out, len)) return NULL;
    const int64_t C = frames > 0 ? emspec_num_columns(frames, n, hop) : 0;
    /* (C <= 0: an invalid format or shape - the library rejects it with its message before it touches any output) */
    if (C > 0 && !stereo_outs_hold(env, out, len, (size_t)sources * (size_t)C * (size_t)h->rows)) return NULL;
    int rc = emspec_batch_pcm_stereo(h->e, src, &fmt, sources, frames, n, hop, reassign ? 1 : 0, a, b, have ? &m : NULL, (float*)out[0],
                                     (uint8_t*)out[1], (uint8_t*)out[2], (uint8_t*)out[3]);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}
static napi_value HistoryViewStereo(napi_env env, napi_callback_info info) {
    size_t argc = 15; napi_value argv[15];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 15) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "historyViewStereo(handle, session, stream0, pairs, views, a, b, firstColumn, factor, groups, map, outLevel, outIndex, outPan, outRgba)");
        return NULL;
    }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t v32[6] = {0}, factor = 0; int64_t first = 0, groups = 0;   /* session, stream0, pairs, views, a, b */
    for (int i = 0; i < 6; ++i) NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1 + i], &v32[i]));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[7], &first));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[8], &factor));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[9], &groups));
    emspec_stereo_map m; int have = 0;
    if (!get_stereo_map(env, argv[10], &m, &have)) return NULL;
    void* out[4]; size_t len[4];
    if (!get_stereo_outs(env, argv + 11, out, len)) return NULL;
    /* (pairs or groups below 1: the library rejects the call with its message before it touches an output) */
    if (v32[2] >= 1 && groups >= 1 && !stereo_outs_hold(env, out, len, (size_t)v32[2] * (size_t)groups * (size_t)h->rows)) return NULL;
    int rc = emspec_history_view_stereo(h->e, v32[0], v32[1], v32[2], v32[3], v32[4], v32[5], first, factor, groups, have ? &m : NULL,
                                        (float*)out[0], (uint8_t*)out[1], (uint8_t*)out[2], (uint8_t*)out[3]);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}

/* Live audio history (include/emspec.h: emspec_set_live_audio / emspec_live_audio / emspec_audio_view / emspec_audio_batch).
 * setLiveAudio(handle, samples): W samples per stream, 0 clears
 * liveAudio(handle, session, stream) -> [end, first] or null (no audio history, or the session has no such stream)
 * audioView(handle, session, stream0, streams, firstSample, count, out:Float32Array(streams * count))
 * audioBatch(handle, session, stream0, streams, firstSample, count, fftSize, hop, reassign, outDb, outRgba, outIndex) -> columns:
 *            each output a typed array of exactly streams * columns * rows cells (RGBA: x 4) or null */
static napi_value SetLiveAudio(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "setLiveAudio(handle, samples)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int64_t w = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[1], &w));
    int rc = emspec_set_live_audio(h->e, w);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
static napi_value LiveAudio(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "liveAudio(handle, session, stream)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t session = 0, stream = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &session));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &stream));
    int64_t first = -1;
    const int64_t end = emspec_live_audio(h->e, session, stream, &first);
    napi_value r;
    if (end < 0) { NAPI_OK_OR_RETURN(env, napi_get_null(env, &r)); return r; }
    napi_value a, b;
    NAPI_OK_OR_RETURN(env, napi_create_array_with_length(env, 2, &r));
    NAPI_OK_OR_RETURN(env, napi_create_int64(env, end, &a));
    NAPI_OK_OR_RETURN(env, napi_create_int64(env, first, &b));
    NAPI_OK_OR_RETURN(env, napi_set_element(env, r, 0, a));
    NAPI_OK_OR_RETURN(env, napi_set_element(env, r, 1, b));
    return r;
}
static napi_value AudioView(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 7) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "audioView(handle, session, stream0, streams, firstSample, count, out)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t session = 0, stream0 = 0, streams = 0; int64_t first = 0, count = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &session));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &stream0));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &streams));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[4], &first));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[5], &count));
    void* out = NULL; size_t olen = 0;
    if (!get_typed(env, argv[6], napi_float32_array, &out, &olen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "out must be a Float32Array"); return NULL; }
    /* (streams or count below 1: the library rejects the call with its message before it touches the output) */
    if (streams >= 1 && count >= 1 && olen != (size_t)streams * (size_t)count) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "out must hold exactly streams*count samples");
        return NULL;
    }
    int rc = emspec_audio_view(h->e, session, stream0, streams, first, count, (float*)out, count);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
static napi_value AudioBatch(napi_env env, napi_callback_info info) {
    size_t argc = 12; napi_value argv[12];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 12) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "audioBatch(handle, session, stream0, streams, firstSample, count, fftSize, hop, reassign, outDb, outRgba, outIndex)");
        return NULL;
    }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    int32_t session = 0, stream0 = 0, streams = 0, n = 0, hop = 0; int64_t first = 0, count = 0; bool reassign = true;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &session));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &stream0));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &streams));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[4], &first));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[5], &count));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[6], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[8], &argv[8]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[8], &reassign));
    void *db = NULL, *rgba = NULL, *idx = NULL; size_t dlen = 0, rlen = 0, ilen = 0;
    if (!get_typed(env, argv[9], napi_float32_array, &db, &dlen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array or null"); return NULL; }
    if (!get_typed(env, argv[10], napi_uint8_array, &rgba, &rlen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outRgba must be a Uint8Array or null"); return NULL; }
    if (!get_typed(env, argv[11], napi_uint8_array, &idx, &ilen, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outIndex must be a Uint8Array or null"); return NULL; }
    const int64_t C = out_columns(h, emspec_num_columns(count, n, hop));
    /* (a range or a shape that yields no column: the library rejects the call with its message before it touches an output) */
    if (streams >= 1 && C >= 1) {
        const size_t cells = (size_t)streams * (size_t)C * (size_t)h->rows;
        if ((db && dlen != cells) || (idx && ilen != cells) || (rgba && rlen != 4 * cells)) {
            napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "every output must hold exactly streams*columns*rows cells (RGBA: x 4)");
            return NULL;
        }
    }
    emspec_out out; memset(&out, 0, sizeof(out));
    out.db = (float*)db; out.rgba = (uint8_t*)rgba; out.index = (uint8_t*)idx;
    int rc = emspec_audio_batch(h->e, session, stream0, streams, first, count, n, hop, reassign ? 1 : 0, &out);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, C, &r));
    return r;
}

static napi_value WaveOf(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 7) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "waveOf(pcm, S, L, fftSize, hop, factor, out)"); return NULL; }
    void *pcm = NULL, *out = NULL; size_t plen = 0, olen = 0;
    if (!get_typed(env, argv[0], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S = 0, n = 0, hop = 0, factor = 0; int64_t L = 0;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[2], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &hop));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &factor));
    if (!get_typed(env, argv[6], napi_float32_array, &out, &olen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "out must be a Float32Array"); return NULL; }
    if (S < 0 || L < 0 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    /* (a shape the library rejects: it does so with its message before it touches the output) */
    const int64_t C = emspec_num_columns(L, n, hop), Cr = C >= 0 ? emspec_reduced_columns(C, factor) : -1;
    if (Cr >= 0 && olen != (size_t)S * (size_t)Cr * 2) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "out must hold exactly S*reducedColumns*2 floats");
        return NULL;
    }
    int rc = emspec_wave_host((const float*)pcm, S, L, n, hop, factor, (emspec_wave*)out);
    if (rc != EMSPEC_OK) return throw_status(env, NULL, rc);
    return NULL;
}
static napi_value PositionHz(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    double pos = 0.0, hz = 0.0;
    if (argc < 2 || napi_get_value_double(env, argv[1], &pos) != napi_ok) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "positionHz(handle, pos)"); return NULL; }
    int rc = emspec_position_hz(h->e, (float)pos, &hz);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_double(env, hz, &r));
    return r;
}

/* allocPinned(byteLength) -> ArrayBuffer backed by page-locked host memory (emspec_host_alloc);
 * typed arrays over it make batch()/column() copies run at full PCIe speed.  Freed by the GC. */
static void finalize_pinned(napi_env env, void* data, void* hint) { (void)env; (void)hint; emspec_host_free(data); }
static napi_value AllocPinned(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int64_t bytes = 0;
    if (argc < 1 || napi_get_value_int64(env, argv[0], &bytes) != napi_ok || bytes <= 0) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "allocPinned(byteLength > 0)"); return NULL; }
    void* p = NULL;
    int rc = emspec_host_alloc((size_t)bytes, &p);
    if (rc != EMSPEC_OK) { napi_throw_error(env, status_name(rc), "page-locked allocation failed"); return NULL; }
    napi_value ab;
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, finalize_pinned, NULL, &ab) != napi_ok) {
        emspec_host_free(p);
        napi_throw_error(env, "EMSPEC_NAPI", "napi_create_external_arraybuffer failed");
        return NULL;
    }
    return ab;
}

static napi_value NumColumns(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int64_t L = 0; int32_t n = 0, hop = 0;
    if (argc < 3) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "numColumns(L, fftSize, hop)"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[0], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &hop));
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_num_columns(L, n, hop), &r));
    return r;
}

/* multiresColumns(L, lowFftSize, fftSize, hop) -> columns of a multi-resolution batch, -1 for a shape it does not accept */
static napi_value MultiresColumns(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int64_t L = 0; int32_t nl = 0, nh = 0, hop = 0;
    if (argc < 4) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "multiresColumns(L, lowFftSize, fftSize, hop)"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[0], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &nl));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &nh));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &hop));
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_multires_columns(L, nl, nh, hop), &r));
    return r;
}

/* multibandColumns(L, fftSizes:Int32Array, hop) -> columns of a multi-band batch, -1 for a shape it does not accept */
static napi_value MultibandColumns(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int64_t L = 0; int32_t hop = 0, K = 0, n[8];
    if (argc < 3 || !get_int32_list(env, argv[1], n, &K)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "multibandColumns(L, fftSizes:Int32Array, hop)"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[0], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &hop));
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, emspec_multiband_columns(L, K, n, hop), &r));
    return r;
}

/* multibandShifts(fftSizes:Int32Array, hop) -> Int32Array of the bands' column shifts, null for a shape that is not accepted */
static napi_value MultibandShifts(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int32_t hop = 0, K = 0, n[8], shifts[8];
    if (argc < 2 || !get_int32_list(env, argv[0], n, &K)) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "multibandShifts(fftSizes:Int32Array, hop)"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &hop));
    napi_value r;
    if (emspec_multiband_shifts(K, n, hop, shifts) != 0) { NAPI_OK_OR_RETURN(env, napi_get_null(env, &r)); return r; }
    napi_value ab; void* data;
    NAPI_OK_OR_RETURN(env, napi_create_arraybuffer(env, (size_t)K * sizeof(int32_t), &data, &ab));
    memcpy(data, shifts, (size_t)K * sizeof(int32_t));
    NAPI_OK_OR_RETURN(env, napi_create_typedarray(env, napi_int32_array, (size_t)K, ab, 0, &r));
    return r;
}

static napi_value LatencyColumns(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    int32_t n = 0, hop = 0; bool re = true;
    if (argc < 2) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "latencyColumns(fftSize, hop[, reassign])"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[0], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[1], &hop));
    if (argc > 2) { NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[2], &argv[2])); NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[2], &re)); }
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int32(env, emspec_latency_columns(n, hop, re ? 1 : 0), &r));
    return r;
}

/* ---- multi-GPU (include/emspec.h "Multi-GPU"): one node process per GPU ---- */
/* commUniqueId() -> Uint8Array(128): rank 0 calls it and hands the bytes to the other rank processes (IPC, a file...) */
static napi_value CommUniqueId(napi_env env, napi_callback_info info) {
    (void)info;
    void* data; napi_value ab, ta;
    NAPI_OK_OR_RETURN(env, napi_create_arraybuffer(env, EMSPEC_COMM_ID_BYTES, &data, &ab));
    if (emspec_comm_unique_id((uint8_t*)data) != EMSPEC_OK) { napi_throw_error(env, "EMSPEC_ERR_COMM", emspec_last_error(NULL)); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_create_typedarray(env, napi_uint8_array, EMSPEC_COMM_ID_BYTES, ab, 0, &ta));
    return ta;
}
/* commInit(handle, id:Uint8Array(128), rank, world): collective over all rank processes */
static napi_value CommInit(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "commInit(handle, id, rank, world)"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* id; size_t len; int32_t rank, world;
    if (!get_typed(env, argv[1], napi_uint8_array, &id, &len, 0) || len != EMSPEC_COMM_ID_BYTES) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "id must be the Uint8Array(128) of commUniqueId()"); return NULL; }
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &rank));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[3], &world));
    int rc = emspec_comm_init(h->e, (const uint8_t*)id, rank, world);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    return NULL;
}
/* batchGather(handle, pcm, S, L, fftSize, hop, reassign, root, outAllIndex?:Uint8Array(world*S*C*rows), outDb?:Float32Array(S*C*rows))
 * -> bytes this rank put on the wire.  Collective: every rank process calls it with its own shard of the streams. */
static napi_value BatchGather(napi_env env, napi_callback_info info) {
    size_t argc = 10; napi_value argv[10];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 8) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "batchGather(handle, pcm, S, L, fftSize, hop, reassign, root[, outAllIndex, outDb])"); return NULL; }
    handle_t* h = get_handle(env, argv[0]); if (!h) return NULL;
    void* pcm; size_t plen;
    if (!get_typed(env, argv[1], napi_float32_array, &pcm, &plen, 0)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm must be a Float32Array"); return NULL; }
    int32_t S, n, hop, root; int64_t L; bool reassign;
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[2], &S));
    NAPI_OK_OR_RETURN(env, napi_get_value_int64(env, argv[3], &L));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[4], &n));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[5], &hop));
    NAPI_OK_OR_RETURN(env, napi_coerce_to_bool(env, argv[6], &argv[6]));
    NAPI_OK_OR_RETURN(env, napi_get_value_bool(env, argv[6], &reassign));
    NAPI_OK_OR_RETURN(env, napi_get_value_int32(env, argv[7], &root));
    if (S < 1 || L < 1 || (size_t)S * (size_t)L != plen) { napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "pcm.length must equal S*L"); return NULL; }
    void *pall = NULL, *pdb = NULL; size_t lall = 0, ldb = 0;
    if (argc > 8 && !get_typed(env, argv[8], napi_uint8_array, &pall, &lall, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outAllIndex must be a Uint8Array"); return NULL; }
    if (argc > 9 && !get_typed(env, argv[9], napi_float32_array, &pdb, &ldb, 1)) { napi_throw_type_error(env, "EMSPEC_ERR_INVALID_ARG", "outDb must be a Float32Array"); return NULL; }
    const int64_t C = out_columns(h, emspec_num_columns(L, n, hop));
    const int32_t world = emspec_comm_world(h->e), rank = emspec_comm_rank(h->e);
    const size_t cells = (size_t)S * (size_t)(C > 0 ? C : 0) * (size_t)h->rows;
    if (world < 1) { napi_throw_error(env, "EMSPEC_ERR_STATE", "no communicator: call commInit first"); return NULL; }
    if (C <= 0 || (rank == root && lall != cells * (size_t)world) || (pdb && ldb != cells)) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "outAllIndex must hold world*S*columns*rows bytes on the root, outDb S*columns*rows floats");
        return NULL;
    }
    int64_t sent = 0;
    int rc = emspec_batch_gather(h->e, (const float*)pcm, S, L, n, hop, reassign ? 1 : 0, root, rank == root ? (uint8_t*)pall : NULL,
                                 (float*)pdb, &sent);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_create_int64(env, sent, &r));
    return r;
}

/* buildInfo() -> "emspec abi=2 sources=<sha16> arch=gfx950" */
static napi_value BuildInfo(napi_env env, napi_callback_info info) {
    (void)info;
    napi_value r;
    NAPI_OK_OR_RETURN(env, napi_create_string_utf8(env, emspec_build_info(), NAPI_AUTO_LENGTH, &r));
    return r;
}

/* deviceStatus(handle): synchronise the device; throws when a kernel flagged a protocol error */
static napi_value DeviceStatus(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK_OR_RETURN(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = NULL;
    if (argc < 1 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !h || !h->e) {
        napi_throw_error(env, "EMSPEC_ERR_INVALID_ARG", "engine handle expected");
        return NULL;
    }
    int rc = emspec_device_status(h->e);
    if (rc != EMSPEC_OK) return throw_status(env, h->e, rc);
    napi_value r; NAPI_OK_OR_RETURN(env, napi_get_undefined(env, &r));
    return r;
}

static napi_value Init(napi_env env, napi_value exports) {
    napi_property_descriptor props[] = {
        {"create", NULL, Create, NULL, NULL, NULL, napi_default, NULL},
        {"destroy", NULL, Destroy, NULL, NULL, NULL, napi_default, NULL},
        {"rows", NULL, Rows, NULL, NULL, NULL, napi_default, NULL},
        {"column", NULL, Column, NULL, NULL, NULL, napi_default, NULL},
        {"flush", NULL, Flush, NULL, NULL, NULL, napi_default, NULL},
        {"push", NULL, Push, NULL, NULL, NULL, napi_default, NULL},
        {"pushColumns", NULL, PushColumns, NULL, NULL, NULL, napi_default, NULL},
        {"warpedEdges", NULL, WarpedEdges, NULL, NULL, NULL, napi_default, NULL},
        {"referenceColormap", NULL, ReferenceColormap, NULL, NULL, NULL, napi_default, NULL},
        {"reset", NULL, Reset, NULL, NULL, NULL, napi_default, NULL},
        {"batch", NULL, Batch, NULL, NULL, NULL, napi_default, NULL},
        {"batchAsync", NULL, BatchAsync, NULL, NULL, NULL, napi_default, NULL},
        {"batchPacked", NULL, BatchPacked, NULL, NULL, NULL, napi_default, NULL},
        {"batchPackedAsync", NULL, BatchPackedAsync, NULL, NULL, NULL, napi_default, NULL},
        {"wireUnpack", NULL, WireUnpack, NULL, NULL, NULL, napi_default, NULL},
        {"wireBound", NULL, WireBound, NULL, NULL, NULL, napi_default, NULL},
        {"setColormap", NULL, SetColormap, NULL, NULL, NULL, napi_default, NULL},
        {"setDisplay", NULL, SetDisplay, NULL, NULL, NULL, napi_default, NULL},
        {"setTimeReduce", NULL, SetTimeReduce, NULL, NULL, NULL, napi_default, NULL},
        {"timeReduce", NULL, TimeReduce, NULL, NULL, NULL, napi_default, NULL},
        {"reducedColumns", NULL, ReducedColumns, NULL, NULL, NULL, napi_default, NULL},
        {"batchPeaks", NULL, BatchPeaks, NULL, NULL, NULL, napi_default, NULL},
        {"peaksOf", NULL, PeaksOf, NULL, NULL, NULL, napi_default, NULL},
        {"setWaveOut", NULL, SetWaveOut, NULL, NULL, NULL, napi_default, NULL},
        {"waveOf", NULL, WaveOf, NULL, NULL, NULL, napi_default, NULL},
        {"setLevelOut", NULL, SetLevelOut, NULL, NULL, NULL, napi_default, NULL},
        {"setCrossOut", NULL, SetCrossOut, NULL, NULL, NULL, napi_default, NULL},
        {"levelsOf", NULL, LevelsOf, NULL, NULL, NULL, napi_default, NULL},
        {"crossOf", NULL, CrossOf, NULL, NULL, NULL, napi_default, NULL},
        {"levelWindow", NULL, LevelWindow, NULL, NULL, NULL, napi_default, NULL},
        {"levelValues", NULL, LevelValues, NULL, NULL, NULL, napi_default, NULL},
        {"crossCorrelation", NULL, CrossCorrelation, NULL, NULL, NULL, napi_default, NULL},
        {"setLivePeaks", NULL, SetLivePeaks, NULL, NULL, NULL, napi_default, NULL},
        {"setLiveWave", NULL, SetLiveWave, NULL, NULL, NULL, napi_default, NULL},
        {"setLiveLevel", NULL, SetLiveLevel, NULL, NULL, NULL, napi_default, NULL},
        {"setLiveCross", NULL, SetLiveCross, NULL, NULL, NULL, napi_default, NULL},
        {"levelSum", NULL, LevelSum, NULL, NULL, NULL, napi_default, NULL},
        {"crossSum", NULL, CrossSum, NULL, NULL, NULL, napi_default, NULL},
        {"setLiveHistory", NULL, SetLiveHistory, NULL, NULL, NULL, napi_default, NULL},
        {"liveHistory", NULL, LiveHistory, NULL, NULL, NULL, napi_default, NULL},
        {"historyView", NULL, HistoryView, NULL, NULL, NULL, napi_default, NULL},
        {"stereoColormap", NULL, StereoColormap, NULL, NULL, NULL, napi_default, NULL},
        {"setStereoColormap", NULL, SetStereoColormap, NULL, NULL, NULL, napi_default, NULL},
        {"batchPcmStereo", NULL, BatchPcmStereo, NULL, NULL, NULL, napi_default, NULL},
        {"historyViewStereo", NULL, HistoryViewStereo, NULL, NULL, NULL, napi_default, NULL},
        {"setLiveAudio", NULL, SetLiveAudio, NULL, NULL, NULL, napi_default, NULL},
        {"liveAudio", NULL, LiveAudio, NULL, NULL, NULL, napi_default, NULL},
        {"audioView", NULL, AudioView, NULL, NULL, NULL, napi_default, NULL},
        {"audioBatch", NULL, AudioBatch, NULL, NULL, NULL, napi_default, NULL},
        {"positionHz", NULL, PositionHz, NULL, NULL, NULL, napi_default, NULL},
        {"setRowEdges", NULL, SetRowEdges, NULL, NULL, NULL, napi_default, NULL},
        {"getRowEdges", NULL, GetRowEdges, NULL, NULL, NULL, napi_default, NULL},
        {"allocPinned", NULL, AllocPinned, NULL, NULL, NULL, napi_default, NULL},
        {"numColumns", NULL, NumColumns, NULL, NULL, NULL, napi_default, NULL},
        {"latencyColumns", NULL, LatencyColumns, NULL, NULL, NULL, napi_default, NULL},
        {"multiresColumns", NULL, MultiresColumns, NULL, NULL, NULL, napi_default, NULL},
        {"batchMultires", NULL, BatchMultires, NULL, NULL, NULL, napi_default, NULL},
        {"multibandColumns", NULL, MultibandColumns, NULL, NULL, NULL, napi_default, NULL},
        {"multibandShifts", NULL, MultibandShifts, NULL, NULL, NULL, napi_default, NULL},
        {"batchMultiband", NULL, BatchMultiband, NULL, NULL, NULL, napi_default, NULL},
        {"commUniqueId", NULL, CommUniqueId, NULL, NULL, NULL, napi_default, NULL},
        {"commInit", NULL, CommInit, NULL, NULL, NULL, napi_default, NULL},
        {"batchGather", NULL, BatchGather, NULL, NULL, NULL, napi_default, NULL},
        {"buildInfo", NULL, BuildInfo, NULL, NULL, NULL, napi_default, NULL},
        {"deviceStatus", NULL, DeviceStatus, NULL, NULL, NULL, napi_default, NULL},
        {"columns", NULL, Columns, NULL, NULL, NULL, napi_default, NULL},
        {"columnsAsync", NULL, ColumnsAsync, NULL, NULL, NULL, napi_default, NULL},
        {"columnsFlush", NULL, ColumnsFlush, NULL, NULL, NULL, napi_default, NULL},
        {"pushMulti", NULL, PushMulti, NULL, NULL, NULL, napi_default, NULL},
        {"pushColumnsMulti", NULL, PushColumnsMulti, NULL, NULL, NULL, napi_default, NULL},
        {"resetStream", NULL, ResetStream, NULL, NULL, NULL, napi_default, NULL},
        {"liveStreams", NULL, LiveStreams, NULL, NULL, NULL, napi_default, NULL},
        {"pcmFrameBytes", NULL, PcmFrameBytes, NULL, NULL, NULL, napi_default, NULL},
        {"batchPcm", NULL, BatchPcm, NULL, NULL, NULL, napi_default, NULL},
        {"batchPcmPacked", NULL, BatchPcmPacked, NULL, NULL, NULL, napi_default, NULL},
        {"pushPcm", NULL, PushPcm, NULL, NULL, NULL, napi_default, NULL},
    };
    napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
