/* libblaze_hip - MI355X (gfx950) device path for blaze's MSM / NTT / Poseidon-tree primitives.
 *
 * C ABI cut at the DriverPrimitive method level: one function per trait method per primitive
 * (reference trait: src/driver_client/dclient.rs:28-46; the three primitives: MSMClient, NTTClient, PoseidonClient).  Each entry cites the reference
 * interface it replaces.  Plain pointers and sizes only; the callee borrows host pointers for the
 * duration of the call; the caller provides output buffers.  A handle is not thread-safe; distinct
 * handles are independent (own stream and workspace).  Nothing here ever falls back to a CPU path:
 * if no HIP device is usable every constructor fails with BLZ_ERR_FILE.
 *
 * Return value of every int function: 0 = Ok, otherwise a DriverClientError code in the order of
 * the reference enum (src/error.rs:6-32); blz_last_error_message() gives the detail string
 * (the `offset` / `path` payload of the reference variants).
 */
#ifndef BLAZE_HIP_H
#define BLAZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/error.rs:6-32, same order */
enum blz_error {
    BLZ_OK = 0,
    BLZ_ERR_WRITE = 1,               /* WriteError{offset,source}: host->device transfer failed      */
    BLZ_ERR_READ = 2,                /* ReadError{offset,source}: device->host transfer failed       */
    BLZ_ERR_HBICAP_NOT_READY = 3,    /* HBICAPNotReady: never produced (no bitstream to load)        */
    BLZ_ERR_INVALID_PARAM = 4,       /* InvalidPrimitiveParam: bad mode combination / sizes / state  */
    BLZ_ERR_CSV = 5,                 /* CsvError: never produced                                     */
    BLZ_ERR_LOAD_FAILED = 6,         /* LoadFailed{path}: librccl.so.1 (comm API) / a Poseidon instruction file could not be loaded */
    BLZ_ERR_FILE = 7,                /* FileError: device could not be opened (no GPU / bad ordinal) */
    BLZ_ERR_UNKNOWN = 8              /* Unknown: kernel launch / runtime failure                     */
};

/* src/ingo_msm/msm_cfg.rs:4-8 and :11-14, declaration order */
enum blz_curve { BLZ_BLS377 = 0, BLZ_BLS381 = 1, BLZ_BN254 = 2 };
enum blz_mem { BLZ_HBM = 0, BLZ_DMA = 1 };

#define BLZ_PRECOMPUTE_FACTOR_BASE 1u /* src/ingo_msm/msm_api.rs:39 */
#define BLZ_PRECOMPUTE_FACTOR 8u      /* src/ingo_msm/msm_api.rs:40 */
#define BLZ_SCALAR_SIZE 32u           /* src/ingo_msm/msm_cfg.rs:48 */

typedef struct blz_msm blz_msm;
typedef struct blz_ntt blz_ntt;
typedef struct blz_poseidon blz_poseidon;

const char* blz_last_error_message(void);
/* number of usable HIP devices (0 when there is none); never fails */
int blz_device_count(void);
/* sizes per curve: src/ingo_msm/msm_cfg.rs:44-92 (point 96/64, result 144/96) */
size_t blz_point_size(int curve);
size_t blz_result_size(int curve);

/* ------------------------------------------------------------------ MSM (src/ingo_msm/msm_api.rs) */

/* DriverClient::new(id, cfg) (dclient.rs:79-86) + MSMClient::new(MSMInit{mem_type,is_precompute,curve})
 * (msm_api.rs:44-55).  (BN254, HBM) is todo!() in the reference (msm_cfg.rs:38); here it is defined
 * by analogy (point 64 B, result 96 B). */
int blz_msm_new(int device_id, int mem_type, int is_precompute, int curve, blz_msm** out);
void blz_msm_free(blz_msm* h);

/* MSMClient::loaded_binary_parameters (msm_api.rs:57-70): [image_id, image_parameters].
 * image_parameters packs the fields of MSMImageParametrs (msm_api.rs:333-347). */
int blz_msm_loaded_binary_parameters(blz_msm* h, uint32_t out[2]);

/* MSMClient::initialize(MSMParams{nof_elements, hbm_point_addr}) (msm_api.rs:72-111).
 * has_hbm=0 <=> hbm_point_addr == None.  mem_type==HBM with has_hbm==0 panics in the reference
 * (unwrap at msm_api.rs:84) -> BLZ_ERR_INVALID_PARAM here. */
int blz_msm_initialize(blz_msm* h, uint32_t nof_elements, int has_hbm, uint64_t hbm_addr, uint64_t hbm_off);

/* MSMClient::start_process (msm_api.rs:113-120): push the configured task to the task queue.
 * The device has a task queue and a result queue (msm_hw_code.rs:19-25): up to TWO tasks may be in
 * flight (initialize / start_process / set_data twice before the first wait_result).  Results are
 * returned in submission order with their labels.  The few-lane tail of a task (upper bucket-reduce
 * levels, Horner, inversion) overlaps the sort + accumulation of the next one, so a stream of MSMs
 * should keep two in flight.  A third submission returns BLZ_ERR_INVALID_PARAM until a result was
 * collected with wait_result; blz_msm_is_engine_ready reports whether a task can be accepted. */
int blz_msm_start_process(blz_msm* h);

/* MSMClient::set_data(MSMInput{points, scalars, params}) (msm_api.rs:155-220).
 *   points == NULL, has_hbm      : scalars only, bases read from the device arena (:163-174)
 *   points != NULL, !has_hbm     : scalars + points streamed (:175-202)
 *   points != NULL, has_hbm      : load_data_to_hbm(points) then scalars (:203-216)
 *   points == NULL, !has_hbm     : silent no-op in the reference (falls through) -> no-op here
 * points_len must be nof_elements * precompute_factor * point_size, scalars_len nof_elements*32.
 * Largest task: points x windows <= 2^32 - 2^26 - 352 321 536 points at precompute_factor 1 (5 x the reference's largest shape;
 * 134 GiB of device memory on BN254), 2^31 - 2^25 points at precompute_factor 8 (2^30 run: 172 GiB); beyond: InvalidPrimitiveParam
 * before anything is copied.  hbm_addr + hbm_off must not wrap around 2^64.
 * Blocking: host buffers may be dropped when it returns (pwrite with O_SYNC, utils.rs:71).
 *
 * STREAMED TASKS.  The reference writes the input to the card's FIFOs in 2048-element chunks (:175-202) and the card counts
 * elements against NUMBER_OF_MSM_ELEMENTS, the register initialize() wrote (msm_hw_code.rs:18-19): a task's bytes may be split
 * over any number of set_data calls.  Same here ({armed_n, received}, launch when received == armed_n): with a
 * task queued (start_process), a set_data whose nof_elements is SMALLER than what the task still lacks is its next slice -
 * lengths are checked against the slice's own nof_elements; any slice sizes (2048-element cadence, ragged tails, zero);
 * every slice in the mode of the first (scalars only: the same hbm_point_addr, the address of the task's FIRST base, in every
 * slice; points + scalars; points + hbm_point_addr: slice k's table is loaded right behind slice k - 1's, its address must say
 * so).  The task is handed to the device piece by piece while later slices are still with the host (the pieces of a one-call
 * DMA-mode task) and is complete with the slice that brings received to nof_elements; more than that is refused and changes
 * nothing, initialize / start_process / wait_result with a half-fed task are refused (its element count is the
 * nof_elements it was armed with when its first slice came; a task already in flight can still be waited for),
 * blz_msm_reset drops it.  A slice that fails in transfer loses the stream: the task stays queued and may be sent again from
 * its first element.  Results are byte-identical to the one-call task's (tests/test_gpu_msm_stream.py).  The reference's
 * largest DMA-mode shape - tests/integration_msm.rs:386-467, 2^26 elements x 8 bases = a 48 GiB host vector - runs from host
 * slices of any size this way.  blz_msm_stream_progress: {elements received, elements of the queued task}. */
int blz_msm_set_data(blz_msm* h, const uint8_t* points, size_t points_len, const uint8_t* scalars,
                     size_t scalars_len, uint32_t nof_elements, int has_hbm, uint64_t hbm_addr,
                     uint64_t hbm_off);

/* Same semantics with inputs already resident in this device's HBM (device pointers, borrowed until
 * wait_result returns; the slices of a streamed task are COPIED into the handle's staging set and may be dropped on
 * return).  No reference counterpart: the FPGA path has no device-pointer notion; this
 * is what a multi-GPU host or a pipeline that produced scalars on the GPU calls. */
int blz_msm_set_data_device(blz_msm* h, const void* d_points, size_t points_len, const void* d_scalars,
                            size_t scalars_len, uint32_t nof_elements, int has_hbm, uint64_t hbm_addr,
                            uint64_t hbm_off);

/* MSMClient::wait_result (msm_api.rs:222-238): block until the OLDEST task's result is valid.
 * The reference spins forever when nothing is armed; here that is BLZ_ERR_INVALID_PARAM.
 * BOUNDED: the reference polls RESULT_VALID without a deadline; every host-side wait of this library (wait_result,
 * the blocking copies of set_data / load_data_to_hbm / result, the exchange) polls against BLAZE_WAIT_TIMEOUT_MS
 * (environment, milliseconds, default 120000).  On expiry the call returns BLZ_ERR_UNKNOWN (message: "... timed
 * out after N ms"), the task stays queued and the handle turns RESET-ONLY: every call except blz_msm_reset /
 * blz_msm_free / blz_msm_result (of results already collected) fails with BLZ_ERR_UNKNOWN until a reset succeeds;
 * reset itself waits, bounded, for the handle's streams to drain.  Same for the NTT handle. */
int blz_msm_wait_result(blz_msm* h);

/* MSMClient::result (msm_api.rs:240-274): read result_point_size bytes + RESULT_LABEL, pop.
 * Layout Z | Y | X, canonical little-endian, homogeneous projective (tests/msm/mod.rs:397-403);
 * this build always emits the normalised point Z=1 (infinity: Z=0, Y=1, X=0). */
int blz_msm_result(blz_msm* h, uint8_t* out, size_t out_cap, size_t* out_len, uint32_t* label);

/* MSMClient::load_data_to_hbm / get_data_from_hbm (msm_api.rs:299-322): raw bytes at arena byte
 * offset addr+off.  The arena is per device and process-global (points persist across handles, as
 * they persist across clients on the card: tests/integration_msm_hbm.rs:51-56) and behaves like the
 * card's flat memory: a write keeps every byte outside its own range, writes that touch or overlap
 * earlier ones form one contiguous extent (a table may be loaded in pieces), and only a range that
 * was never written cannot be read or used as bases. */
int blz_msm_load_data_to_hbm(blz_msm* h, const uint8_t* points, size_t len, uint64_t addr, uint64_t off);
int blz_msm_load_data_to_hbm_device(blz_msm* h, const void* d_points, size_t len, uint64_t addr, uint64_t off);
int blz_msm_get_data_from_hbm(blz_msm* h, uint8_t* out, size_t len, uint64_t addr, uint64_t off);
/* drop every arena extent of a device (no reference counterpart; the card keeps HBM until reset) */
int blz_arena_release(int device_id);
/* Arena policy (per device, process-wide; default 0).  BLZ_ARENA_DROP_RAW: an extent keeps its bytes as loaded AND a Montgomery
 * copy of the points the tasks gather from (BLS: 96 + 128 bytes per base; 48 + 64 GiB for the reference's largest precompute
 * shape) although only get_data_from_hbm, a later write, an export or a table build ever read the former.  With the bit set,
 * once an extent's copy is complete and every coordinate has been seen to be canonical (< q: such points convert to Montgomery
 * form and back without loss; an extent that holds one that is not keeps its bytes), the raw bytes are freed; whoever needs them
 * again gets them converted back - get_data_from_hbm returns the same bytes as before, a write / blz_arena_export /
 * window-table build / precompute-table check first restores the whole extent (one pass).  Not applied to extents shared with
 * other processes, to extents whose point grid does not start at their first byte, under handles that asked for a window table,
 * or to the even-base copy of a checked precompute table (which is not the whole table).  blz_msm_memory_info shows the effect. */
#define BLZ_ARENA_DROP_RAW 1u
int blz_arena_set_policy(int device_id, uint32_t policy);
/* Cross-process arena (the card's HBM outlives the process that loaded it; GPU memory does not, so a holder
 * process keeps it): blz_arena_export writes one IPC handle per extent of this process to `registry_path`;
 * blz_arena_attach, in ANOTHER process, maps those extents at the same arena offsets (all of them or, on any
 * failure, none), after which hbm_point_addr / get_data_from_hbm address the holder's bytes.  Shared extents are
 * READ-ONLY on both sides from the export on (every process keeps a private Montgomery copy of the points and
 * tracks staleness locally): load_data_to_hbm into one returns WriteError, in the holder too; a load that only
 * touches one starts a separate extent.  blz_arena_release un-shares.  The extents live as long as the holder
 * does.  (HSA_ENABLE_IPC_MODE_LEGACY=0 where the host driver only supports dmabuf IPC.) */
int blz_arena_export(int device_id, const char* registry_path);
int blz_arena_attach(int device_id, const char* registry_path);

/* The HIP stream (hipStream_t, as void*) the handle's tasks are enqueued on, and its device ordinal (nullable): a host that
 * produces scalars - or consumes results - with kernels of its own orders them against the handle's tasks with events on this
 * stream instead of host-side waits.  The driver client of the reference holds file descriptors (dclient.rs:50-59); this is
 * their GPU counterpart.  The stream stays the library's: do not destroy it. */
int blz_msm_stream(blz_msm* h, void** hip_stream, int* device_id);
/* MSMClient::task_label / nof_elements / is_msm_engine_ready (msm_api.rs:278-297) */
int blz_msm_task_label(blz_msm* h, uint32_t* out);
int blz_msm_nof_elements(blz_msm* h, uint32_t* out);
int blz_msm_is_engine_ready(blz_msm* h, uint32_t* out);
/* streamed tasks (blz_msm_set_data): out = {elements the queued task has received so far, elements it was queued with}; {0, 0}
 * with nothing queued.  Diagnostic (the card's FIFO fill is not readable at all). */
int blz_msm_stream_progress(blz_msm* h, uint32_t out[2]);
/* DriverClient::reset (dclient.rs:88-93): drop armed task, queued results and staged data. */
int blz_msm_reset(blz_msm* h);

/* Phase timers of the last completed task, milliseconds (the device clock counters of
 * msm_hw_code.rs:35-46 LAST_TASK_PHASE{1,2,3}_TOTAL_CLOCKS read through get_api, msm_api.rs:324-330):
 * [0] whole device pipeline  [1] k_accumulate kernel alone  [2] digit sort (count+scan+scatter)
 * [3] bucket accumulation (phase 1)  [4] bucket reduce (phase 2)  [5] window combine + affine (phase 3)
 * [6] window bits c  [7] number of windows */
int blz_msm_last_timings(blz_msm* h, float out[8]);
/* 1 when the digit sort of the last completed task ran underneath the accumulation of the task before it (two tasks in
 * flight, the sort's kernels fit beside the accumulation's waves: DESIGN.md section 3), else 0.  Diagnostic. */
int blz_msm_last_sort_hidden(blz_msm* h, int* out);

/* Device memory behind a handle, bytes (get_api, msm_api.rs:324-330, dumps the card's registers; the one figure a GPU host
 * needs that the card never had to report): out = {engine workspace (grown to the largest task seen), staging buffers of this
 * handle, arena: raw bytes as loaded (allocated), arena: Montgomery copies of the bases, arena: window tables + build scratch,
 * total}.  The three arena figures are per DEVICE (every handle of the device reports the same). */
int blz_msm_memory_info(blz_msm* h, uint64_t out[6]);

/* precompute_base_* (tests/msm/mod.rs:360-380) on the device: for each of the n base points (x||y)
 * write PRECOMPUTE_FACTOR = 8 points P, 2^32 P, ..., 2^224 P contiguously to d_out (n*8 points).
 * The reference builds this table on the host before set_data / load_data_to_hbm. */
int blz_msm_precompute_bases_device(int device_id, int curve, const void* d_points, void* d_out, uint64_t n);

/* The window plan the pipeline would use for this input size (no device needed): out = {widest lower
 * window in bits, windows W, unit length L, bucket slots G}; widths (nullable, room for 96 bytes)
 * receives the W window widths, low to high.  The widths always sum to at least the scalar width + 1
 * (signed digits).  Diagnostic; no reference counterpart (the bitstream's plan is fixed). */
int blz_msm_plan(int curve, uint32_t nof_elements, int is_precompute, uint32_t out[4], uint8_t* widths);

/* Resident-base window table (opt-in; no reference counterpart - the closest is the caller-supplied x8 table of
 * MSMInit.is_precompute, msm_api.rs:40-50, which costs 16 window passes per element where the plain path needs 12).
 * enable: 0 off, 1 on where it was measured to pay (BLS12-377 / BLS12-381; BN254's 64-byte points are already
 * gathered at the memory system's rate and lose 4 % with a table, so 1 leaves BN254 on the plain path), 2 always.
 * With it, a pf = 1 handle whose bases live in the arena (hbm_point_addr) builds the table of their window multiples
 * 2^(c j) P, j < W = ceil(257 / c) - 1.9 s of the chip for 2^26 BLS12-381 bases, paced by the tasks (below), W x the memory
 * of the Montgomery copy (2^26: 10 x 8 GiB) - and keeps it with the arena extent: a later write of up to 2^18 bases has their rows
 * re-tabulated ahead of the next task, a larger one drops the table (the tasks that follow rebuild it).  Tasks over
 * those bases then add every window's digit into ONE bucket set:
 * 10 windows of 26 bits at 2^26 (671 M bucket additions, 2^25 buckets) instead of 12 windows of 21-23 bits (805 M).
 * Results are bit-identical to the plain path's.  Falls back to the plain path (silently; BLAZE_LOG=1 says why) when
 * the table does not fit the free memory, when a base has even order (a multiple at infinity cannot be tabulated;
 * never the case in the r-torsion), or for a task over a sub-range that wants a different window width.
 * A handle with a scalar range (blz_msm_set_scalar_range) tabulates 2^(bit_lo + c j) P for the windows of its range.
 * New handles start UNSET, which is neither of the three: the library decides (the auto policy).  An unset pf = 1 handle of
 * PointMemoryType HBM on a BLS curve gets the table of its resident bases when a task of at least 2^24 bases is the second
 * scalars-only task in a row over the identical bases and scalar range with no write in between, and the table takes at most
 * half of the device memory free at that moment.  That build is not paced: all of it is enqueued at once on the handle's stream
 * ahead of the triggering task (2.3 s of the chip for 2^26 bases: one late result; the host call does not wait), and the first
 * task launched after it has completed adopts the table.  A table built this way is given back when an allocation of the
 * library fails for lack of device memory (the extent then stays on the plain path until its next write); tables built under 1
 * or 2 are the caller's decision and stay.  Calling this function with 0 is an explicit off; 1 and 2 keep their meaning and
 * their paced build.  BLAZE_MSM_PLAN keys steer the policy: auto_table=0 switches it off for the process, auto_table_min=N sets
 * the least number of bases, table_budget_bytes=N replaces the half-of-free rule by an absolute cap.
 * No other value of `enable` is accepted (InvalidPrimitiveParam). */
int blz_msm_set_window_table(blz_msm* h, int enable);
/* The table's build is never one lump inside a task: it is cut into chunks of 196 608 bases (~5.5 ms of the chip), every task
 * launched over the bases first enqueues four of them on its own stream and takes the plain path, like every task until the
 * last chunk has completed; the next task adopts the table.  Results are bit-identical either way.  A host that wants the
 * table in place before its first task calls this after load_data_to_hbm: it allocates the table (do this with the load: an
 * 80 GiB hipMalloc takes 0.3 ms on a clean device and seconds on one that has memory to scrub), enqueues the first chunks
 * (wait_ms = 0) or ALL the remaining ones (wait_ms != 0) for the nof_elements bases at hbm_addr + hbm_off and waits up to
 * wait_ms (< 0: BLAZE_WAIT_TIMEOUT_MS) for the build; *ready = 1 when the table is in place, 0 otherwise (still building, not opted in, no memory, a base of even
 * order, another handle's table serves the extent). */
int blz_msm_prepare_window_table(blz_msm* h, uint32_t nof_elements, uint64_t hbm_addr, uint64_t hbm_off, int wait_ms, int* ready);
/* out = {table bytes, window bits c, windows W, build time in microseconds} of the table the handle's last HBM task
 * used; zeros when it took the plain path */
int blz_msm_window_table_info(blz_msm* h, uint64_t out[4]);

/* Checked-table plan for precompute handles (opt-in; MSMInit.is_precompute, msm_api.rs:39-50).  The reference's precompute mode
 * has the CALLER supply, per element, the 8 bases B_j = 2^(32 j) P (precompute_base_*: tests/msm/mod.rs:360-380) and defines the
 * task as sum_i sum_j s_(i,j) B_(i,j) over the 32-bit chunks of the scalars.  Served literally - the default - that is an 8n-point
 * MSM of 32-bit scalars: 16 bucket additions per element where the same elements without a table need 12.  With enable = 1 a
 * handle whose bases live in the arena (hbm_point_addr) CHECKS the table once per load - on the device, base by base: B_(i,0) on the
 * curve and B_(i,j) == 2^32 B_(i,j-1) for j = 1..7 (32 doublings each, compared projectively; 0.7 s for 2^26 BN254 elements,
 * 1.3 s on the BLS curves) - and, if it holds, sums sum_i sum_k (s_(i,2k) + 2^32 s_(i,2k+1)) B_(i,2k) instead: 4n points with 64-bit
 * scalars, three windows of 22 / 22 / 21 bits, 12 additions per element into 3 shared bucket sets, over a Montgomery copy of
 * the even bases only (half the copy's memory).  The two sums are the same group element exactly when the check holds, and the
 * result is emitted normalised (Z = 1), so the bytes are identical to the exact path's.  A table that fails the check (any base
 * off the curve, any multiple that is not 2^32 times its predecessor, a multiple at infinity) keeps the exact path - silently;
 * BLAZE_LOG=1 says so, blz_msm_precompute_plan_info reports it.  A write into a consistent table has the next task check the elements
 * it touched (only those); a write into a refuted one, the whole range again.  The check runs inside the first set_data / start_process that launches a task over the bases (the call blocks
 * for it), or in blz_msm_prepare_precompute_plan for a host that wants to pay with the load.  Tasks that bring their own points
 * (DMA mode, and set_data with points AND an hbm address) always take the exact path: they are link-bound, and a check per task
 * would cost more than it saves.
 * New handles start with 0.  InvalidPrimitiveParam for a handle without is_precompute. */
int blz_msm_set_precompute_plan(blz_msm* h, int enable);
/* run the check (and build the even-base copy) now for the nof_elements elements at hbm_addr + hbm_off; *consistent = 1 when
 * tasks over them will take the plan, 0 otherwise (not opted in, table refuted, bases off the extent's element grid) */
int blz_msm_prepare_precompute_plan(blz_msm* h, uint32_t nof_elements, uint64_t hbm_addr, uint64_t hbm_off, int* consistent);
/* out = {1 if the handle's last HBM task took the plan, state of the check of its bases (0 not asked / not checked, 1 consistent,
 * 2 refuted), device time of the check in microseconds, bytes of the even-base Montgomery copy} */
int blz_msm_precompute_plan_info(blz_msm* h, uint64_t out[4]);

/* Sharding by scalar chunk (multi-GPU; no reference counterpart - README.md:20-22 leaves the split to a "management
 * layer").  A handle with a scalar range sums only bits [bit_lo, bit_hi) of every scalar it is given and returns
 * 2^bit_lo x that sum: the partial results of the ranges of a partition of [0, 256) add up to the full MSM, like the partial
 * results of element chunks do (blz_msm_combine_partials / blz_msm_all_gather_combine), and the two splits compose.
 * Why: Pippenger's cost per rank is (elements x windows) additions + (windows x 2^(c-1)) bucket slots to reduce, and a rank
 * that gets 1/8 of the ELEMENTS has to narrow its windows (2^23 elements: 15 windows of 19 bits - 126 M additions) where a
 * rank that gets 1/4 of the elements' BITS for half of the elements keeps the big job's windows (2^25 elements x 3
 * windows of 22 bits - 101 M).  32-bit aligned ranges, precompute_factor 1; (0, 0) or (0, 256) = the whole scalar. */
int blz_msm_set_scalar_range(blz_msm* h, uint32_t bit_lo, uint32_t bit_hi);
/* The split blz picks for `nranks` equal devices: out = {first element, element count, bit_lo, bit_hi} of `rank`.
 * R ranges of 256 / R bits x nranks / R element chunks, R in {1, 2, 4, 8} dividing nranks, chosen by the window planner's
 * cost estimate of a rank's task; rank = chunk * R + range.  BLAZE_SHARD=elements forces the element split (R = 1),
 * BLAZE_SHARD=bits the largest R.  Host-side only (no device needed). */
int blz_msm_shard_layout(int curve, uint32_t nof_elements, int nranks, int rank, uint32_t out[4]);
/* The same choice with the flow's transfers priced in.  A split into R scalar ranges makes the R ranks of a range group need
 * the SAME element chunk: R x the scalar bytes per rank on its PCIe link when the scalars come from host memory with every
 * task (the reference's HBM flow, tests/integration_msm_hbm.rs:57-100), R x the bases per rank in device memory - and on
 * the link too when the bases travel with every task (DMA flow).  With t = bytes over the rank's link / 56 GB/s (measured)
 * and c = the window planner's compute estimate, cost(R) = max(c + 0.15 t, 1.1 t) per task (a stream of tasks overlaps the
 * two, not for free: profiles/r04_shard_layouts.txt), and a layout whose per-rank bases and scalars exceed half of the
 * device memory is not considered.  R > 1 is taken only when it beats the element split by more than
 * 2 % (the simpler layout wins ties).  flags: BLZ_SHARD_SCALARS_FROM_HOST, BLZ_SHARD_BASES_FROM_HOST; 0 = everything
 * resident (what blz_msm_shard_layout prices).  out = {first element, element count, bit_lo, bit_hi, R, estimated compute us,
 * estimated link us, device MiB per rank (bases raw + Montgomery copy + scalars)}.  Host-side only. */
#define BLZ_SHARD_SCALARS_FROM_HOST 1u
#define BLZ_SHARD_BASES_FROM_HOST 2u
int blz_msm_shard_layout_ex(int curve, uint32_t nof_elements, int nranks, int rank, uint32_t flags, uint32_t out[8]);
/* the estimates of one candidate (R ranges) for tools and tests: out as above; InvalidPrimitiveParam if R does not divide nranks */
int blz_msm_shard_layout_candidate(int curve, uint32_t nof_elements, int nranks, int rank, uint32_t flags, int R, uint32_t out[8]);

/* Multi-GPU: add G partial results (each result_size bytes, as returned by blz_msm_result on each
 * rank, in rank order) on this handle's device and emit the normalised sum, for hosts that move the
 * partials themselves (blz_msm_all_gather_combine below does the exchange too). */
int blz_msm_combine_partials(blz_msm* h, const uint8_t* partials, size_t count, uint8_t* out, size_t out_cap);

/* Multi-GPU exchange inside the library (one process per GPU, or one handle per device of one process): an
 * RCCL communicator rank per handle, then  all-gather of the ranks' partial results over xGMI + rank-ordered
 * add on the device + normalise, so every rank returns the same bytes.  (RCCL's reduce operators are
 * arithmetic, not a group law: all-gather + local add instead of all-reduce)  The reference
 * leaves the multi-device layer to a "management layer" (README.md:20-22); this is that layer for a Rust / C++
 * host.  RCCL is resolved at run time (dlopen of librccl.so.1); without it these return LoadFailed.
 *   rank 0:        blz_comm_unique_id(id); the host ships the 128 bytes to the other ranks (MPI, a file, a pipe ...)
 *   every rank:    blz_msm_comm_init(h, rank, nranks, id)                        -- collective
 *   per MSM:       blz_msm_result(h, partial ...); blz_msm_all_gather_combine(h, partial, out, cap) -- collective
 *   every rank:    blz_msm_comm_free(h)   (blz_msm_free does it too)
 * One process driving several devices from one thread (one handle per device, rank i = handles[i]):
 *   once:          blz_msm_comm_init_all(handles, n)                             -- one RCCL group (ncclGroupStart/End)
 *   per MSM:       blz_msm_all_gather_combine_all(handles, n, partials, out, cap) -- partials / out: n x result_size
 * (blz_msm_comm_init / blz_msm_all_gather_combine are blocking rendezvous: called for several handles from ONE
 * thread they would wait for each other - use the _all forms there.)
 * Deadlines: the bring-up runs against BLAZE_COMM_TIMEOUT_MS (default 60000) and fails with BLZ_ERR_UNKNOWN when a
 * peer never arrives; the exchange is a bounded wait like wait_result (BLAZE_WAIT_TIMEOUT_MS). */
#define BLZ_COMM_ID_BYTES 128
int blz_comm_unique_id(uint8_t out[BLZ_COMM_ID_BYTES]);
int blz_msm_comm_init(blz_msm* h, int rank, int nranks, const uint8_t id[BLZ_COMM_ID_BYTES]);
int blz_msm_all_gather_combine(blz_msm* h, const uint8_t* partial, uint8_t* out, size_t out_cap);
int blz_msm_comm_init_all(blz_msm* const* handles, int n);
int blz_msm_all_gather_combine_all(blz_msm* const* handles, int n, const uint8_t* partials, uint8_t* out, size_t out_cap);
int blz_msm_comm_free(blz_msm* h);

/* ------------------------------------------------------------------ NTT (src/ingo_ntt/ntt_api.rs) */

/* DriverClient::new + NTTClient::new(NTT::Ntt, dclient) (ntt_api.rs:26-31).  log_size = 27 is the
 * reference shape (ntt_data.rs:65); smaller sizes exist for tests.  Field: BLS12-381 Fr
 * (BASELINE.json), forward transform, natural order in/out, omega = 2^log_size-th root derived from
 * the multiplicative generator 7. */
int blz_ntt_new(int device_id, int log_size, blz_ntt** out);
/* same, with the transform direction: inverse != 0 gives x[i] = n^-1 sum_k X[k] omega^(-ik) (natural order;
 * the reference has no such knob: SURVEY.md 8(f) rank 3) */
int blz_ntt_new_ex(int device_id, int log_size, int inverse, blz_ntt** out);
/* same over the scalar field of another curve (field = enum blz_curve: BLS12-377 Fr, generator 22,
 * two-adicity 47; BN254 Fr, generator 5, two-adicity 28).  The bitstream the
 * reference drives is built for one field; here the kernels are instantiated per field. */
int blz_ntt_new_field(int device_id, int field, int log_size, int inverse, blz_ntt** out);
/* same, with flags.  BLZ_NTT_NO_FACTOR_TABLE: never allocate the per-element boundary-factor table of a 2^27 transform's
 * second pass (n x 32 bytes: 4 GiB beside the handle's 12 GiB of buffers): the pass steps the factors along each lane's rows
 * instead - the kernel a memory-tight device gets anyway (the table is an optimisation worth ~2 %, allocated when it fits) and the
 * one every smaller transform runs.  blz_ntt_info says which one a handle got. */
#define BLZ_NTT_NO_FACTOR_TABLE 1u
int blz_ntt_new_ex2(int device_id, int field, int log_size, int inverse, uint32_t flags, blz_ntt** out);
/* The transform's CONVENTION, chosen by the caller.  The reference states none of it (NttInit {} is empty, ntt_api.rs:8-23; its
 * golden files are external, tests/integration_ntt.rs:15-18): this build's default is X[k] = sum_i x[i] w^(i k) with
 * w = g^((r - 1) / 2^log_size), g the field's multiplicative generator (7 / 22 / 5 for BLS12-381 / BLS12-377 / BN254 Fr), natural
 * order in and out.  A host that holds vectors made for the card says here what they assume:
 *   root   (nullable) 32 bytes, canonical little-endian: ANY primitive 2^log_size-th root of unity replaces w; checked on the
 *          device (root < r and root^(2^(log_size - 1)) == -1), else BLZ_ERR_INVALID_PARAM;
 *   flags  BLZ_NTT_NO_FACTOR_TABLE as above; BLZ_NTT_INVERSE: x = n^-1 sum_k X[k] w^(-i k) (the same w: the inverse of the
 *          handle without the flag); BLZ_NTT_BITREV_INPUT / BLZ_NTT_BITREV_OUTPUT: position p of the buffer passed to
 *          set_data / returned by result holds the element of index bitrev(p) over log_size bits (the orders decimation-in-time
 *          inputs / decimation-in-frequency outputs come in) - folded into the first pass's loads and the last pass's stores.
 * Handles made without root and order flags are byte-identical to blz_ntt_new_ex2's. */
#define BLZ_NTT_INVERSE 2u
#define BLZ_NTT_BITREV_INPUT 4u
#define BLZ_NTT_BITREV_OUTPUT 8u
int blz_ntt_new_ex3(int device_id, int field, int log_size, uint32_t flags, const uint8_t* root, blz_ntt** out);
/* Coset transforms.  shift = 32 bytes, canonical little-endian, a field element g with 0 < g < r;
 * NULL (or g = 1) = the plain transform again.
 *   handle without BLZ_NTT_INVERSE:  X[k] = sum_i x[i] g^i w^(i k)       (evaluate on the coset g<w>)
 *   handle with    BLZ_NTT_INVERSE:  x[i] = g^(-i) n^-1 sum_k X[k] w^(-i k)   (its exact inverse)
 * i and k are LOGICAL indices: with BLZ_NTT_BITREV_INPUT / _OUTPUT the buffers are permuted as before,
 * the power of g follows the element, not the buffer position.  w is the handle's root (default or
 * the caller's).  Fused into the transform's passes: no pass over the data and no launch is added.
 * Blocking; rebuilds only the tables that carry g (among them, at 2^27, pass 2's per-element factor table
 * where the handle has one); leaves both transform buffers' contents alone; holds for transforms started
 * after it returns and across blz_ntt_reset.  BLZ_ERR_INVALID_PARAM, changing nothing: null handle, shift = 0,
 * shift >= r (checked on the device), a transform in flight on the handle. */
int blz_ntt_set_coset(blz_ntt* h, const uint8_t* shift);
/* the shift in force: 32 bytes, the element 1 when the handle runs the plain transform */
int blz_ntt_get_coset(blz_ntt* h, uint8_t out[32]);
/* out = {device bytes the handle holds (two transform buffers + scratch + twiddle / factor tables), 1 if pass 2 reads the
 * per-element factor table / 0 if it steps its factors, 1 if pass 1 reads the column-independent boundary table, log_size} */
int blz_ntt_info(blz_ntt* h, uint64_t out[4]);
void blz_ntt_free(blz_ntt* h);
/* NTTClient::initialize(NttInit{}) (ntt_api.rs:37-56) */
int blz_ntt_initialize(blz_ntt* h);
/* NTTClient::set_data(NTTInput{buf_host, data}) (ntt_api.rs:72-87): data = 2^log_size x 32 B LE, canonical field
 * elements; a word >= r is taken as the residue it represents (the output is canonical either way) */
int blz_ntt_set_data(blz_ntt* h, size_t buf_host, const uint8_t* data, size_t len);
int blz_ntt_set_data_device(blz_ntt* h, size_t buf_host, const void* d_data, size_t len);
/* NTTClient::start_process(Some(buf_kernel)) (ntt_api.rs:58-70): in-place transform of that buffer */
int blz_ntt_start_process(blz_ntt* h, size_t buf_kernel);
/* NTTClient::wait_result (ntt_api.rs:89-108) */
int blz_ntt_wait_result(blz_ntt* h);
/* NTTClient::result(Some(buf)) (ntt_api.rs:110-124) */
int blz_ntt_result(blz_ntt* h, size_t buf, uint8_t* out, size_t out_cap);
int blz_ntt_result_device(blz_ntt* h, size_t buf, void* d_out, size_t out_cap);
/* NTTClient::result(Some(buf)) followed by NTTClient::set_data(NTTInput{buf_host: buf, data}) - what every cycle of the
 * reference's double-buffered loop does while the kernel runs on the other buffer (tests/integration_ntt.rs:102-136) - as ONE
 * call that drives the link in both directions at once: the buffer leaves for prev_out piece by piece and next_in lands in the
 * places that have left.  Same preconditions as the two calls (the buffer must not be under transform); blocking; both host
 * buffers may be dropped / read when it returns.  in_len = 2^log_size x 32, out_cap >= that. */
int blz_ntt_exchange(blz_ntt* h, size_t buf, const uint8_t* next_in, size_t in_len, uint8_t* prev_out, size_t out_cap);
/* the HIP stream (hipStream_t, as void*) the handle's transforms run on, and its device ordinal (nullable); see blz_msm_stream */
int blz_ntt_stream(blz_ntt* h, void** hip_stream, int* device_id);
/* DriverClient::reset (dclient.rs:88-93) without the 100 ms sleep */
int blz_ntt_reset(blz_ntt* h);
/* kernel time of the last transform in ms (what benches/ntt_bench.rs:34-39 times, minus reset()) */
int blz_ntt_last_kernel_ms(blz_ntt* h, float* out);
/* Element-wise ops on resident buffers: the "combine" step between two transforms (a quotient polynomial is
 * evaluate on g<w>, combine point by point, interpolate back) without a trip through the host.  Over the handle's field,
 * n = 2^log_size elements, position by position: dst[p] = op(a[p], b[p], c[p]).
 *   Values: every input word is any 256-bit value and counts as its residue (the transforms' rule); every output word is
 *   canonical (< r), little-endian.  BLZ_VEC_INV maps 0 (and r, 2r ...) to 0.
 *   Operands: d_ptr == NULL names the handle's transform buffer `buf` (count 0 or n); otherwise d_ptr is device memory of the
 *   handle's device, 16-byte aligned, holding `count` 32-byte elements, count a power of two, 1 <= count <= n, and position
 *   p of the op reads element p & (count - 1): count = 1 is a scalar, count = 4 carries the four values of 1 / Z_H on a 4x
 *   domain, count = n is a vector.  The period runs along the buffer POSITION p: the handle's BLZ_NTT_BITREV_* flags and
 *   its coset shift play no part here, the op sees positions, not logical indices.
 *   dst is the transform buffer buf_dst and may be a buffer an operand names (in place); a and b may be the same (a square).
 *   Operands an op does not take must be NULL, operands it takes must not be.
 *   Protocol: that of a transform.  The op is enqueued on the handle's compute stream and the call returns;
 *   blz_ntt_wait_result finishes it (bounded, as for a transform) and blz_ntt_last_kernel_ms then reports its device time.
 *   Until then buf_dst may not be read, written or exchanged, the transform buffers the op READS may be read
 *   (blz_ntt_result) but not written or exchanged, and blz_ntt_start_process, blz_ntt_set_coset and another
 *   blz_ntt_vec_op are refused.  Memory behind a d_ptr must stay valid and unwritten until blz_ntt_wait_result returns: the
 *   library does not copy it.  blz_ntt_reset drops an op in flight like a transform.
 *   BLZ_ERR_INVALID_PARAM, before anything is enqueued: null handle, unknown op, buf_dst > 1, buf > 1, reserved != 0, a
 *   count that is zero, not a power of two or above n (d_ptr == NULL: neither 0 nor n), a missing or surplus operand, a d_ptr
 *   the runtime does not know as device memory of the handle's device, or one that is not 16-byte aligned. */
enum blz_vec_op { BLZ_VEC_ADD = 0,     /* dst = a + b     */
                  BLZ_VEC_SUB = 1,     /* dst = a - b     */
                  BLZ_VEC_MUL = 2,     /* dst = a * b     */
                  BLZ_VEC_MULADD = 3,  /* dst = a * b + c */
                  BLZ_VEC_MULSUB = 4,  /* dst = a * b - c */
                  BLZ_VEC_INV = 5 };   /* dst = a^-1, and 0 -> 0 (batch inversion) */
typedef struct blz_vec_arg {
    const void* d_ptr;   /* NULL: the handle's transform buffer `buf`; else device memory on the handle's device */
    uint32_t buf;        /* 0 | 1, read only when d_ptr == NULL */
    uint32_t reserved;   /* must be 0 */
    uint64_t count;      /* d_ptr != NULL: number of 32-byte elements, a power of two, 1 <= count <= n (the source of
                            blz_ntt_vec_gather, _scatter and _spmv: <= 2^27); position p of the op reads element p & (count - 1).
                            d_ptr == NULL: 0 or n */
} blz_vec_arg;
int blz_ntt_vec_op(blz_ntt* h, int op, size_t buf_dst, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c);
/* Reductions and prefix scans on resident buffers: the folds ALONG the buffer that blz_ntt_vec_op, position by position,
 * cannot express - a polynomial evaluated at a challenge point, an inner product, a sum check (one value out of a vector);
 * the grand-product column Z[p + 1] = Z[p] num[p] / den[p], a lookup argument's running sums, the powers z^p (a running
 * product or sum).  Over the handle's field, on the n = 2^log_size positions p = 0 .. n - 1.
 *   Values: every input word is any 256-bit value and counts as its residue; every output word is canonical (< r),
 *   little-endian.  Nothing is special-cased for zeros: a zero (or r, 2r ...) in a product scan makes every later position 0
 *   (BLZ_VEC_INV, which maps 0 to 0, is the only op that treats zeros apart).
 *   Operands: those of blz_ntt_vec_op, checked by the same code - a transform buffer, or `count` device words read at
 *   p & (count - 1).  The ops see buffer POSITIONS: the handle's BLZ_NTT_BITREV_* flags and its coset shift play no part.
 *   BLZ_FOLD_SUM takes no b.  BLZ_FOLD_EVAL takes the point z as b with d_ptr != NULL and count == 1; z stays on the device,
 *   the host never reads it; 0^0 = 1, so z = 0 gives a[0].
 *   Scan: inclusive dst[p] = a[0] o .. o a[p]; with BLZ_SCAN_EXCLUSIVE dst[0] = the identity (0 for SUM, 1 for PROD) and
 *   dst[p] = a[0] o .. o a[p - 1].  dst is the transform buffer buf_dst and may be the buffer a names (in place).  Hence an
 *   exclusive BLZ_SCAN_PROD of a one-word operand z writes the powers dst[p] = z^p.
 *   d_out / d_total: 32 bytes of device memory on the handle's device, 16-byte aligned, checked like an operand's d_ptr,
 *   not overlapping the words of a d_ptr operand, written only by the op.  d_total may be NULL; otherwise it receives the
 *   fold of all n elements (the last inclusive value, whatever the flag).
 *   Protocol: that of blz_ntt_vec_op.  Everything is checked before anything is enqueued; the op runs on the compute stream
 *   and the call returns without waiting for the device; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports
 *   it, blz_ntt_reset drops it.  While a scan is in flight buf_dst may not be read, written or exchanged.  A reduce writes no
 *   transform buffer: the buffers it reads may be read but not written or exchanged, a buffer it does not name stays free.
 *   While either is in flight blz_ntt_start_process, blz_ntt_set_coset, blz_ntt_vec_op, blz_ntt_vec_reduce and
 *   blz_ntt_vec_scan are refused.  Memory behind d_ptr, d_out and d_total stays valid (d_ptr: unwritten) until
 *   blz_ntt_wait_result returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: null handle, unknown op, unknown flag bits, buf_dst > 1, a missing or surplus
 *   operand, EVAL with b naming a transform buffer or with count != 1, null d_out, a d_out / d_total that is not such
 *   memory or overlaps a d_ptr operand, and any operand error of blz_ntt_vec_op. */
enum blz_fold_op { BLZ_FOLD_SUM = 0,    /* out = sum_p a[p]                              */
                   BLZ_FOLD_DOT = 1,    /* out = sum_p a[p] * b[p]                       */
                   BLZ_FOLD_EVAL = 2 }; /* out = sum_p a[p] * z^p, z = b (count must be 1; 0^0 = 1) */
int blz_ntt_vec_reduce(blz_ntt* h, int op, const blz_vec_arg* a, const blz_vec_arg* b, void* d_out);
enum blz_scan_op { BLZ_SCAN_SUM = 0, BLZ_SCAN_PROD = 1 };
#define BLZ_SCAN_EXCLUSIVE 1u
int blz_ntt_vec_scan(blz_ntt* h, int op, uint32_t flags, size_t buf_dst, const blz_vec_arg* a, void* d_total);
/* Weighted (Horner) scan on resident buffers: the recurrence dst[p] = a[p] + z dst[p -+ 1] with a one-word multiplier z, in
 * either direction, inclusive or exclusive - the half of a KZG-style opening that blz_ntt_vec_reduce(BLZ_FOLD_EVAL) leaves:
 * the witness polynomial q(X) = (f(X) - f(z)) / (X - z) by synthetic division.  Over the handle's field, on the n = 2^log_size
 * buffer POSITIONS (the BLZ_NTT_BITREV_* flags and the coset shift play no part).
 *   flags 0                        dst[p] = a[p] + z dst[p - 1] = sum_{j <= p} a[j] z^(p - j)
 *   BLZ_HORNER_EXCLUSIVE           dst[p] = sum_{j < p} a[j] z^(p - 1 - j), dst[0] = 0
 *   BLZ_HORNER_REVERSE             dst[p] = a[p] + z dst[p + 1] = sum_{j >= p} a[j] z^(j - p)
 *   BLZ_HORNER_REVERSE | EXCLUSIVE dst[p] = sum_{j > p} a[j] z^(j - p - 1), dst[n - 1] = 0: the n coefficients of the quotient
 *                                  of a(X) by X - z (EXCLUSIVE alone: the same for a polynomial stored top coefficient first)
 *   d_total (nullable) receives the last inclusive value whatever the flags: forward sum_j a[j] z^(n - 1 - j), reverse
 *   sum_j a[j] z^j = a(z), the division's remainder.  0^0 = 1 and nothing is special-cased: with z = 0 the inclusive scan
 *   copies a and the exclusive scan shifts it by one position; z = 1 gives prefix / suffix sums.
 *   Values: every input word is any 256-bit value and counts as its residue; every output word is canonical, little-endian.
 *   Operands: a as for blz_ntt_vec_op (a transform buffer, or `count` device words read at p & (count - 1)); dst is the
 *   transform buffer buf_dst and may be the buffer a names.  z follows BLZ_FOLD_EVAL's rule: d_ptr != NULL, count == 1, and the
 *   host never reads it.  d_total: as for blz_ntt_vec_scan, and off the words of a and of z.
 *   Protocol: that of blz_ntt_vec_scan.  Everything is checked before anything is enqueued; the op runs on the compute stream and
 *   the call returns; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports it, blz_ntt_reset drops it.  While it
 *   is in flight buf_dst may not be read, written or exchanged, a buffer that is only read may be read, and
 *   blz_ntt_start_process, blz_ntt_set_coset, blz_ntt_vec_op, blz_ntt_vec_reduce, blz_ntt_vec_scan and blz_ntt_vec_horner are
 *   refused (as blz_ntt_vec_horner is while any of those is in flight).
 *   BLZ_ERR_INVALID_PARAM, changing nothing: null handle, flag bits other than the two, buf_dst > 1, a null a or z, a z that
 *   names a transform buffer or has count != 1, a bad d_total, and any operand error of blz_ntt_vec_op. */
#define BLZ_HORNER_EXCLUSIVE 1u
#define BLZ_HORNER_REVERSE   2u
int blz_ntt_vec_horner(blz_ntt* h, uint32_t flags, size_t buf_dst, const blz_vec_arg* a, const blz_vec_arg* z, void* d_total);
/* Gathers on resident buffers: the one op that moves an element to another POSITION, or between vectors of different length -
 * what every other op, reading position p (or p & (count - 1)) and writing position p, cannot do.  With it the steps of a
 * PLONK-style quotient stay on the device: Z(wX) next to Z(X) (a rotation by 1 on the domain, by 4 on the 4n coset), a
 * low-degree extension (n coefficients into a 4n handle, zero above), the low n coefficients of a 4n result back into an n
 * handle, the values on H out of the evaluations on the 4n domain (every 4th position).  Over the handle's field, by buffer
 * POSITION (the BLZ_NTT_BITREV_* flags and the coset shift play no part), with n = 2^log_size:
 *   dst[p] = a[(offset + stride p) mod count]   for p <  len
 *   dst[p] = 0                                  for len <= p < n
 *   Values: every source word is any 256-bit value and counts as its residue; every output word is canonical, little-endian:
 *   a canonicalising copy.
 *   Source a: a transform buffer (d_ptr == NULL, count 0 or n: count = n) or `count` device words, checked as for
 *   blz_ntt_vec_op with ONE difference: count may exceed n, up to 2^27 (the largest log_size a handle accepts), so that a 4n
 *   vector feeds an n handle.
 *   Index: count is a power of two, so the index is (offset + stride * p) & (count - 1) in 64-bit arithmetic (the wrap at 2^64
 *   is harmless) and nothing is special-cased: stride = count - 1 walks backwards (a reversal with offset = count - 1), stride
 *   = 0 broadcasts one word, len > count tiles the source, an even stride reads some words more than once.  A stride that is 1
 *   modulo count (rotation, extension, slice) reads the source contiguously apart from the wrap; any other stride reads it as
 *   the memory system serves words `stride` apart.
 *   In place: a may name buf_dst.  A gather cannot be done lane by lane, so it then goes through the handle's scratch (n x 32
 *   bytes, nothing else is in flight) and is copied to the buffer on the same stream: twice the traffic of buffer 0 -> buffer
 *   1.  Nothing is allocated and the buffers stay where they are.
 *   Protocol: that of blz_ntt_vec_scan.  Everything is checked before anything is enqueued; the op runs on the compute stream and
 *   the call returns without waiting for the device; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports it,
 *   blz_ntt_reset drops it.  While it is in flight buf_dst may not be read, written or exchanged, a buffer that is only read
 *   may be read, and every transform, blz_ntt_set_coset and op on the buffers is refused (as blz_ntt_vec_gather is while any
 *   of those is in flight).  Memory behind d_ptr stays valid and unwritten until blz_ntt_wait_result returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: null handle, null a or v, buf_dst > 1, offset >= count, len > n, and any operand
 *   error of blz_ntt_vec_op (reserved != 0 among them) with the count bound raised to 2^27. */
typedef struct blz_vec_view {
    uint64_t offset;   /* source element that destination position 0 reads; offset < count */
    uint64_t stride;   /* source step per destination position, taken modulo count */
    uint64_t len;      /* positions p < len read the source, positions len <= p < n become 0; len <= n */
} blz_vec_view;
int blz_ntt_vec_gather(blz_ntt* h, size_t buf_dst, const blz_vec_arg* a, const blz_vec_view* v);
/* Scatter-add on resident buffers: the one op in which a nonzero names the position it is ADDED TO - every other op computes a
 * destination word from the sources that word names.  Not injective and data-dependent, so no inverse table turns it into a
 * gather: the multiplicity column m[t] = #{p : idx[p] = t} of a lookup argument (logUp, Lasso-style memory checking; the
 * indices depend on the witness), and the transposed sparse product A^T y of Spartan's second sumcheck, A(r_x, .) = A^T eq(r_x, .):
 * dst[col[k]] += val[k] * y[row(k)].  Over the handle's field, by buffer POSITION (the BLZ_NTT_BITREV_* flags and the coset shift
 * play no part), with n = 2^log_size:
 *   dst[t] = sum over k < nnz with (idx[k] mod n) == t of val[k] * x[src(k) mod count]   for every t < n
 *   src(k) = d_src ? d_src[k] : k
 *   Without d_val every coefficient is 1; without x every x word is 1; without both it is the histogram: dst[t] is the number
 *   of nonzeros that name t, as a field element.  A position no nonzero names becomes 0.
 *   Values: every word of x and of val is any 256-bit value and counts as its residue; every output word is canonical,
 *   little-endian.  The result is exact in the field and does not depend on the order in which the device adds: two runs give
 *   the same bytes.
 *   x: NULL - ones, and then d_src must be NULL too - or a transform buffer (d_ptr == NULL) or `count` device words, checked as
 *   for blz_ntt_vec_gather: count is a power of two up to 2^27 and may be below or above n; it is read at src(k) & (count - 1), so
 *   a one-word x is a scalar.  x may NOT name buf_dst (nor may its device words overlap that buffer): the destination is the
 *   accumulator.
 *   Indices: idx[k] is taken modulo n and src[k] modulo count (an AND each).  The host never reads the arrays: whatever bytes
 *   they hold, no memory outside the arrays, the destination buffer and the handle's scratch is touched.
 *   Bounds: nnz <= 2^31; nnz = 0 is valid and writes zeros.  The workspace is the handle's scratch (n x 32 bytes); nothing is
 *   allocated.
 *   Pointers: d_idx and d_src are 4-byte aligned device memory of the handle's device with nnz * 4 bytes inside one allocation;
 *   d_val is 16-byte aligned with nnz * 32 bytes.
 *   Cost: the limbs of a term are added into 64-bit integer accumulators with the device's atomic adds, two 64-byte requests at
 *   the memory side per nonzero (one 4-byte add for the histogram); a destination of n <= 1024 (histogram: n <= 16384) is
 *   accumulated in on-chip memory first ("Scatter-add").
 *   Protocol: that of blz_ntt_vec_spmv.  Everything is checked before anything is enqueued; the op runs on the compute stream
 *   and the call returns without waiting for the device; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports
 *   it, blz_ntt_reset drops it.  While it is in flight buf_dst may not be read, written or exchanged, a buffer that is only read
 *   may be read, and every transform, blz_ntt_set_coset and op on the buffers is refused (as blz_ntt_vec_scatter is while any of
 *   those is in flight).  Memory behind the pointers stays valid and unwritten until blz_ntt_wait_result returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: null handle (before any other argument is looked at), null s, buf_dst > 1,
 *   reserved != 0, nnz > 2^31, null d_idx with nnz > 0, d_src given without x, a bad pointer (alignment, not device memory of the
 *   handle's device, the array running past its allocation), x naming or overlapping buf_dst, an op in flight, and any operand
 *   error of blz_ntt_vec_op with the count bound raised to 2^27. */
typedef struct blz_vec_scatter {
    const uint32_t* d_idx;     /* nnz entries: nonzero k is added to position idx[k] mod n (an AND) */
    const uint32_t* d_src;     /* NULL: nonzero k reads x[k mod count]; else nnz entries, x[src[k] mod count] */
    const void*     d_val;     /* NULL: every coefficient is 1; else nnz 32-byte words */
    uint64_t        nnz;       /* <= 2^31; 0 is valid and writes zeros */
    uint64_t        reserved;  /* must be 0 */
} blz_vec_scatter;             /* 40 bytes */
int blz_ntt_vec_scatter(blz_ntt* h, size_t buf_dst, const blz_vec_arg* x, const blz_vec_scatter* s);
/* Sparse matrix-vector products on resident buffers: a sparse matrix in CSR form times a resident vector, into a transform
 * buffer - the first step of a prover, which turns a witness w into vectors on the evaluation domain: A w, B w, C w of an R1CS
 * (one row per constraint, a few nonzeros per row, a tail of very long rows), the wire columns a[p] = w[ia[p]] of PLONK, the
 * looked-up column t[idx[p]] of a lookup argument, a permutation held as an index table (a scatter with known indices is a gather
 * by the inverse table).  Over the handle's field, by buffer POSITION (the BLZ_NTT_BITREV_* flags and the coset shift play no
 * part), with n = 2^log_size:
 *   dst[p] = sum over row_ptr[p] <= k < row_ptr[p + 1] of val[k] * x[col[k] mod count]   for p < rows (an empty row gives 0)
 *   dst[p] = 0                                                                           for rows <= p < n
 *   Values: every word of x and of val is any 256-bit value and counts as its residue; every output word is canonical,
 *   little-endian.
 *   x: a transform buffer (d_ptr == NULL) or `count` device words, checked as for blz_ntt_vec_gather: count is a power of two
 *   up to 2^27 and may be below or above n.  col[k] is taken modulo count (an AND): no column value reaches outside x.
 *   x may NOT name buf_dst (nor may its device words overlap that buffer): the handle's scratch is the op's workspace, so the
 *   gather's detour through it is not available.
 *   Index mode, d_row_ptr == NULL: rows must equal nnz and row p holds nonzero p alone: dst[p] = val[p] * x[col[p] mod count], the
 *   data-dependent gather; with d_val == NULL as well a canonicalising copy without a product.
 *   row_ptr contract: nondecreasing, row_ptr[rows] <= nnz.  Nonzeros below row_ptr[0] or from row_ptr[rows] on belong to no row
 *   and are ignored, so a slab of rows is d_row_ptr + r0 with the full col / val arrays.  The host never reads the arrays and
 *   cannot verify the contract: the kernels clamp every nonzero index to nnz, keep every row index below rows and mask every
 *   column, so whatever bytes row_ptr and col hold, no memory outside the four arrays, the destination buffer and the handle's
 *   scratch is touched.  For arrays that break the contract dst is UNSPECIFIED.
 *   Bounds: rows <= n; nnz <= max(1024, 256 n) and nnz <= 2^31 (the workspace is the handle's scratch, n x 32 bytes, 128 bytes per
 *   tile of 1024 nonzeros; nothing is allocated).  nnz = 0 and rows = 0 are valid and write zeros.
 *   Pointers: d_row_ptr and d_col are 4-byte aligned device memory of the handle's device with (rows + 1) * 4 and nnz * 4 bytes
 *   inside one allocation; d_val is 16-byte aligned with nnz * 32 bytes.
 *   Cost: the work is split by nonzeros, not by rows, so that a long row is spread over lanes and blocks like short ones; the
 *   sums of rows that cross a block's 1024 nonzeros are added up by one lane per row ("Sparse
 *   products": derived from the code's shape, no time is claimed).  The random 32-byte reads of x fetch whole cache lines.
 *   Protocol: that of blz_ntt_vec_gather.  Everything is checked before anything is enqueued; the op runs on the compute stream
 *   and the call returns without waiting for the device; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports
 *   it, blz_ntt_reset drops it.  While it is in flight buf_dst may not be read, written or exchanged, a buffer that is only read
 *   may be read, and every transform, blz_ntt_set_coset and op on the buffers is refused (as blz_ntt_vec_spmv is while any of
 *   those is in flight).  Memory behind the four pointers stays valid and unwritten until blz_ntt_wait_result returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: null handle, null x or m, buf_dst > 1, rows > n, nnz above its bound, null d_col
 *   with nnz > 0, d_row_ptr == NULL with rows != nnz, a bad pointer (alignment, not device memory of the handle's device, the
 *   array running past its allocation), x naming buf_dst, and any operand error of blz_ntt_vec_op with the count bound raised
 *   to 2^27. */
typedef struct blz_vec_csr {
    const uint32_t* d_row_ptr; /* rows + 1 entries; NULL: row p holds nonzero p alone (then rows == nnz) */
    const uint32_t* d_col;     /* nnz entries: nonzero k reads x[col[k] mod count] */
    const void*     d_val;     /* NULL: every coefficient is 1; else nnz 32-byte words */
    uint64_t        rows;      /* <= n; positions rows <= p < n become 0 */
    uint64_t        nnz;
} blz_vec_csr;                 /* 40 bytes */
int blz_ntt_vec_spmv(blz_ntt* h, size_t buf_dst, const blz_vec_arg* x, const blz_vec_csr* m);
/* Multilinear tables on resident buffers: the three steps a sumcheck prover (Spartan, HyperPlonk, GKR) repeats log n times on
 * the vectors blz_ntt_vec_spmv produces - bind a variable, take the round polynomial, build eq(tau, .).  A multilinear polynomial
 * in m variables is its 2^m values on the hypercube, by buffer POSITION p = sum x_i 2^i (the BLZ_NTT_BITREV_* flags and the coset
 * shift play no part); len = 2^m is the live length of a call, 2 <= len <= n, and may shrink from call to call.
 *   blz_ntt_vec_mle_fold   dst[p] = lo + r (hi - lo) for p < len / 2, with (lo, hi) = (a[p], a[p + len / 2]): the TOP variable is
 *                          bound to r; with BLZ_MLE_LOW (lo, hi) = (a[2p], a[2p + 1]): variable 0 is bound.  out_len = len / 2.
 *   blz_ntt_vec_mle_round  out[t] = sum_{p < len / 2} prod_{j < k} (lo_j + t (hi_j - lo_j)) for t = 0 .. points - 1: the round
 *                          polynomial of the product of k tables at the points 0, 1, 2, 3; pairing as in the fold.  k = 1 .. 3 is
 *                          the number of operands, given as a, then b, then c, the ones not taken NULL (b NULL with c set is
 *                          refused); the same table may be named twice.  points = 1 .. 4 is independent of k: a gate that is a
 *                          sum of products of different degrees is one call per product at the same `points`, and the outputs add
 *                          (or ONE blz_ntt_sumcheck_gate, below).
 *                          out[0] + out[1] is the sum (k = 1) or the dot product (k = 2) of the live prefix.
 *   blz_ntt_vec_mle_eq     dst[p] = prod_{i < m} (x_i tau_i + (1 - x_i)(1 - tau_i)) for p < 2^m, tau_i = word i of d_point, x_i =
 *                          bit i of p.  0 <= m <= log_size; m = 0 writes the single word 1.  out_len = 2^m.
 *   Values: every input word (tables, r, the point) is any 256-bit value and counts as its residue; every output word is canonical,
 *   little-endian.
 *   Table operands: those of blz_ntt_vec_op, checked by the same code - a transform buffer, or `count` device words (a power of
 *   two <= n) read at p & (count - 1).
 *   Destination (fold, eq): a blz_vec_arg too.  d_ptr == NULL names transform buffer `buf`; otherwise it names `count` device
 *   words, count a power of two with out_len <= count <= n.  The op writes EXACTLY out_len words from the start of the destination;
 *   every other byte of it keeps its value - no zero fill: a sumcheck's tables shrink geometrically, and so does its traffic.
 *   In place (fold): the destination must start at the same word as the source or not overlap the words the op reads (the first
 *   min(count, len) of a).  In place with the default pairing costs nothing extra; with BLZ_MLE_LOW it goes through the handle's
 *   scratch and a device-to-device copy of len / 2 words on the compute stream.  A periodic source (count < len) cannot be folded in
 *   place.
 *   r: one device word, BLZ_FOLD_EVAL's rule (d_ptr != NULL, count == 1); the host never reads it, so a challenge derived on the
 *   device chains rounds without a round trip.  It may not lie in the words written.
 *   d_out (round): points x 32 bytes of device memory, checked as blz_ntt_vec_reduce's d_out is and off the words of every d_ptr
 *   operand; exactly `points` words are written.  The round writes no transform buffer.
 *   d_point (eq): m x 32 bytes of device memory on the handle's device, 16-byte aligned, inside one allocation, off the words
 *   written; not looked at when m == 0.  The host never reads it.
 *   Cost ("Multilinear tables"; derived from the code): the fold takes one Montgomery product per output
 *   word, the round points x (k - 1) per pair (none at k = 1), the equality table about two per word.
 *   Protocol: that of blz_ntt_vec_op.  Everything is checked before anything is enqueued; the op runs on the compute stream and the
 *   call returns without waiting for the device; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports it,
 *   blz_ntt_reset drops it.  One op is in flight at a time.  While it is, a destination BUFFER may not be read, written or
 *   exchanged, a buffer that is only read may be read, and every transform, blz_ntt_set_coset and op on the buffers is refused.
 *   Memory behind every pointer stays valid (inputs: unwritten) until blz_ntt_wait_result returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: null handle, unknown flag bits, a null a, r, dst, d_out or (m > 0) d_point, an op in
 *   flight, any operand error of blz_ntt_vec_op (dst included); fold: len not a power of two in [2, n], r naming a buffer or with
 *   count != 1, a destination count below out_len, a destination overlapping the source without starting where it starts, in
 *   place with a periodic source, r inside the words written; round: points outside 1 .. 4, b NULL while c is set, a bad d_out or
 *   one that overlaps a d_ptr operand, len as for the fold; eq: m above log_size, a bad d_point or one inside the words written. */
#define BLZ_MLE_LOW 1u
int blz_ntt_vec_mle_fold(blz_ntt* h, uint32_t flags, const blz_vec_arg* dst, const blz_vec_arg* a, const blz_vec_arg* r, uint64_t len);
int blz_ntt_vec_mle_round(blz_ntt* h, uint32_t flags, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c, uint32_t points,
                          uint64_t len, void* d_out);
int blz_ntt_vec_mle_eq(blz_ntt* h, const blz_vec_arg* dst, const void* d_point, uint32_t m);
/* NTTBanks::preprocess / postprocess (ntt_data.rs:80-156) as device permutations, for byte
 * compatibility with bank files of the FPGA flow; n = 2^log_size elements (log_size >= 10), 16 banks
 * contiguous (n/16 elements each); 2^27 uses the reference's 512 groups x 256 block pairs, smaller sizes
 * scale the group count (n >> 18, at least 1). */
int blz_ntt_banks_preprocess_device(blz_ntt* h, const void* d_in, void* d_banks);
int blz_ntt_banks_postprocess_device(blz_ntt* h, const void* d_banks, void* d_out);
/* A sumcheck step on resident tables: bind the top variable of every table to r and take the NEXT round polynomial in the same
 * pass - the fold's output is the round's input, so one op reads each table once where a blz_ntt_vec_mle_fold per table and the
 * blz_ntt_vec_mle_round calls behind them read the folded halves again - and a fourth operand, so that eq (Az o Bz - Cz) is one
 * gate.  Everything is over the handle's field, by buffer POSITION, with the top-variable pairing of blz_ntt_vec_mle_fold
 * ((T[p], T[p + len / 2]); BLZ_MLE_LOW is not offered: fused and in place a lane would write words another lane still reads).
 *   Gates: BLZ_GATE_PRODUCT  G = a, a b or a b c - k = 1 .. 3 tables given as a, then b, then c; d must be NULL;
 *          BLZ_GATE_R1CS     G = a (b c - d) - all four tables.
 *   r != NULL - bind, then round.  r is one device word under BLZ_FOLD_EVAL's rule (d_ptr != NULL, count == 1); the host never
 *     reads it.  Every table T given is folded IN PLACE: T[p] = T[p] + r (T[p + len / 2] - T[p]) for p < len / 2 - exactly len / 2
 *     words of each table are written, every other byte keeps its value.  Then
 *       d_out[t] = sum_{p < len / 4} G(.., T_j[p] + t (T_j[p + len / 4] - T_j[p]), ..) for t < points,
 *     which is what blz_ntt_vec_mle_round at length len / 2 returns on the folded tables.  len >= 4, 1 <= points <= 4.
 *     points == 0 with d_out == NULL is a bind alone: all k tables folded in one op, len >= 2, the gate ignored apart from its
 *     operand-count rule - a sumcheck's last variable.
 *   r == NULL - round only, a sumcheck's first round: d_out[t] = sum_{p < len / 2} G(.. lo_j + t (hi_j - lo_j) ..) with the pairs
 *     (T[p], T[p + len / 2]).  No table is written; len >= 2, 1 <= points <= 4; periodic tables (count < len) are allowed, as in
 *     blz_ntt_vec_mle_round.
 *   Values: any 256-bit input word counts as its residue; every word written - table words and d_out alike - is canonical,
 *   little-endian.  Tables are blz_vec_arg operands, checked by blz_ntt_vec_op's code.
 *   A sumcheck of m variables is blz_ntt_vec_mle_eq, a step without r, m - 1 steps with r, and a bind alone: m + 2 ops.
 *   Cost ("Sumcheck step"; derived from the code): with r each table's len words are read and len / 2
 *   written, once; Montgomery products per quad of four input words per table: 2 k for the folds, plus points x (k - 1)
 *   (PRODUCT) or 2 + 2 points (R1CS: 18 at 4 points, against 20 in the six ops the step replaces).
 *   Protocol: that of blz_ntt_vec_mle_fold.  Everything is checked before anything is enqueued; the op runs on the compute
 *   stream; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms then reports it, blz_ntt_reset drops it.  With r BOTH
 *   transform buffers may be tables and are then both written: while the op is in flight neither may be read, written or
 *   exchanged.  Without r the buffers named are read-only, as for a reduce.  Memory behind every pointer stays valid until
 *   blz_ntt_wait_result returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: a null handle (refused before any other argument is looked at), an unknown gate, a
 *   missing or surplus table, points above 4, points == 0 without r or with a d_out, a null d_out with points > 0, len not a
 *   power of two in [2, n] ([4, n] for a bind and a round), r naming a buffer or with count != 1, an op in flight, any operand
 *   error of blz_ntt_vec_op, a bad d_out or one that overlaps a d_ptr operand; with r: a table with count < len, two tables whose
 *   first len words overlap (the same table named twice is an overlap), r inside the words written, d_out inside the first len
 *   words of a table. */
#define BLZ_GATE_PRODUCT 0u   /* G = a, a b or a b c (k = 1 .. 3 tables; d must be NULL) */
#define BLZ_GATE_R1CS    1u   /* G = a (b c - d)     (all four tables) */
int blz_ntt_sumcheck_step(blz_ntt* h, uint32_t gate, const blz_vec_arg* a, const blz_vec_arg* b, const blz_vec_arg* c,
                          const blz_vec_arg* d, const blz_vec_arg* r, uint32_t points, uint64_t len, void* d_out);
/* The same step for a CALLER-DEFINED gate: a common factor times a signed sum of products of tables,
 *     G = T[common] x sum_{m < nterms} (+/-) prod_{j < nfactors_m} T[factor_mj]        (common == -1: no common factor)
 * which is what a PLONK zerocheck eq (qL a + qR b + qM a b - qO c + qC), a GKR layer add (x + y) + mul x y or a batched Spartan
 * second sumcheck need: up to BLZ_GATE_MAX_TABLES tables, BLZ_GATE_MAX_TERMS terms of up to BLZ_GATE_MAX_FACTORS factors (the
 * common factor not counted) and BLZ_GATE_MAX_POINTS points, in ONE op fused with the bind.  The gate is data, not code: the
 * description below is read on the host, checked, and handed to one kernel.
 *   Layout (fixed; mirrored byte for byte by blaze_amd/_lib.py, include/blaze.hpp and rust/src/driver_client/hip_ffi.rs):
 *     blz_gate_term, 8 bytes:  0 nfactors (1 .. 4) | 1 negate (0: added, 1: subtracted) | 2 .. 5 factor[4], table indices, the
 *       first nfactors are read | 6 .. 7 reserved, must be 0.
 *     blz_sum_gate, 80 bytes:  0 ntables (1 .. 12) | 4 nterms (1 .. 8) | 8 common (-1, or a table index) | 12 reserved, must
 *       be 0 | 16 term[8], the first nterms are read.
 *   A table index may repeat inside a term (a a) and across terms, and common may also be a factor.  tables[] holds ntables
 *   operands; messages name them tables[i].
 *   Semantics: those of blz_ntt_sumcheck_step with G in the gate's place.
 *   r != NULL - bind, then round: EVERY table of tables[] is folded in place, T[p] = T[p] + r (T[p + len / 2] - T[p]) for
 *     p < len / 2, once, whether a term names it or not (tables that only ride along are bound by the same op) - exactly len / 2
 *     words of each are written, every other byte keeps its value.  Then
 *       d_out[t] = sum_{p < len / 4} G(.., T_j[p] + t (T_j[p + len / 4] - T_j[p]), ..) for t < points.
 *     len >= 4, 1 <= points <= BLZ_GATE_MAX_POINTS whatever the gate's degree.  points == 0 with d_out == NULL is a bind alone
 *     (len >= 2): one fold per table in the one op; the description is still checked.
 *   r == NULL - round only: d_out[t] = sum_{p < len / 2} G(.. lo_j + t (hi_j - lo_j) ..) over the pairs (T[p], T[p + len / 2]).
 *     Nothing is written to a table; periodic tables (count < len) are allowed - a constant selector is a one-word table.
 *   Values: any 256-bit input word counts as its residue; every word written - table words and d_out alike - is canonical,
 *   little-endian.
 *   Cost ("Caller-defined gates"; derived from the code): with r each table's len words are read and
 *   len / 2 written, once, and the lane's own two folded words are read again (from cache) once per time a term or common names
 *   the table.  Montgomery products per quad: 2 ntables for the folds, plus per term of f factors points x (f - 1) and
 *   2 (F - f), F the longest term's f, plus points for a common factor: R1CS as common = eq, + Az Bz, - Cz is 8 + 6 + 4 = 18
 *   at 4 points, BLZ_GATE_R1CS's count; the PLONK gate above, 9 tables at 5 points, 58.
 *   Protocol, in-flight rules and operand checks: blz_ntt_sumcheck_step's, by the same code.  With r both transform buffers may
 *   be tables and neither may then be read, written or exchanged until blz_ntt_wait_result; without r the buffers named are
 *   read-only.  Memory behind every pointer stays valid until blz_ntt_wait_result returns; the description is copied.
 *   BLZ_ERR_INVALID_PARAM, changing nothing: a null handle (refused before any other argument is looked at), a null gate or
 *   tables, ntables outside 1 .. 12, nterms outside 1 .. 8, common below -1 or not below ntables, a term's nfactors outside
 *   1 .. 4, negate above 1, a factor index not below ntables, a nonzero reserved byte, points above 6, points == 0 without r or
 *   with a d_out, a null d_out with points > 0, len not a power of two in [2, n] ([4, n] for a bind and a round), r naming a
 *   buffer or with count != 1, an op in flight, any operand error of blz_ntt_vec_op, a bad d_out or one that overlaps a d_ptr
 *   operand; with r: a table with count < len, two tables whose first len words overlap, r inside the words written, d_out
 *   inside the first len words of a table. */
#define BLZ_GATE_MAX_TABLES  12
#define BLZ_GATE_MAX_TERMS    8
#define BLZ_GATE_MAX_FACTORS  4   /* per term, the common factor not counted */
#define BLZ_GATE_MAX_POINTS   6
typedef struct blz_gate_term {
    uint8_t nfactors;                       /* 1 .. BLZ_GATE_MAX_FACTORS */
    uint8_t negate;                         /* 0: the term is added, 1: subtracted */
    uint8_t factor[BLZ_GATE_MAX_FACTORS];   /* table indices; the first nfactors are read */
    uint8_t reserved[2];                    /* must be 0 */
} blz_gate_term;
typedef struct blz_sum_gate {
    uint32_t ntables;    /* 1 .. BLZ_GATE_MAX_TABLES */
    uint32_t nterms;     /* 1 .. BLZ_GATE_MAX_TERMS */
    int32_t common;      /* -1: none; else the table every term is multiplied by */
    uint32_t reserved;   /* must be 0 */
    blz_gate_term term[BLZ_GATE_MAX_TERMS];   /* the first nterms are read */
} blz_sum_gate;
int blz_ntt_sumcheck_gate(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* tables, const blz_vec_arg* r, uint32_t points,
                          uint64_t len, void* d_out);
/* PRODUCT AND FRACTION TREES over a multilinear table: every layer of the binary tree under len = 2^m words, in one op - what a
 * GKR-style argument builds before its first sumcheck.  Layer 0 is the source, read at p & (count - 1); layer k, 1 <= k <= m,
 * holds len / 2^k words, with (lo, hi) = (L_k[p], L_k[p + size_k / 2]) - the top variable, the pairing of the step ops - or
 * (L_k[2p], L_k[2p + 1]) with BLZ_MLE_LOW:
 *   BLZ_TREE_PROD  L_{k+1}[p] = lo hi: the grand product of a permutation or memory check (HyperPlonk, Quarks, Spartan, Lasso).
 *                  Takes dst and a; dst_q and a_q are NULL.
 *   BLZ_TREE_FRAC  pairs (P, Q): P' = P_lo Q_hi + P_hi Q_lo, Q' = Q_lo Q_hi - the sum of fractions of logUp-GKR down to ONE
 *                  fraction, never inverted and with no special case for a zero denominator.  P from a to dst, Q from a_q to
 *                  dst_q; all four are required.  A one-word a holding 1 is the numerator of sum 1 / (beta + f).
 *   Layout: layer k sits at word len - len / 2^(k - 1) of its destination - layer 1 at 0, layer 2 at len / 2, the root at
 *   len - 2.  EXACTLY len - 1 words are written; word len - 1 and everything behind it keep their bytes.  With the default
 *   pairing the two halves of a layer are contiguous power-of-two runs of device words: blz_ntt_sumcheck_gate and the other step
 *   ops take them as tables (d_ptr into the destination) unchanged.
 *   len = 2^m, 2 <= len <= n (blz_ntt_vec_mle_fold's live length).  Sources: operands as for blz_ntt_vec_op, periodic ones allowed.
 *   Destinations: blz_ntt_vec_mle_fold's destination rule with len - 1 words written - a transform buffer, or the caller's
 *   device words, count a power of two with len - 1 <= count <= n; both may be the two transform buffers.  A destination may not meet
 *   the words the op reads of any source (min(count, len)), nor the other destination's len - 1 words: there is no in-place form.
 *   Values: any 256-bit input word counts as its residue; every word written is canonical, little-endian.
 *   Cost ("Product and fraction trees"; derived from the code): 2 Montgomery products per PROD node, 5 per
 *   FRAC node; the leaves are read once and a launch keeps 3 (PROD) or 2 (FRAC) layers in registers: about 2.14 len words moved
 *   for PROD, 4.67 len for FRAC.  No workspace.
 *   Protocol, in-flight rules and operand checks: blz_ntt_vec_mle_fold's, by the same code; a destination buffer is the buffer
 *   written.  BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing: a null handle (refused before any other argument
 *   is looked at), an unknown op, unknown flag bits, a missing or surplus operand for the op, len not 2^m in [2, n], an op in
 *   flight, any operand error of blz_ntt_vec_op in a source or a destination, a destination count below len - 1, and the
 *   overlaps above. */
enum blz_tree_op { BLZ_TREE_PROD = 0, BLZ_TREE_FRAC = 1 };
int blz_ntt_mle_tree(blz_ntt* h, uint32_t op, uint32_t flags, const blz_vec_arg* dst, const blz_vec_arg* dst_q, const blz_vec_arg* a,
                     const blz_vec_arg* a_q, uint64_t len);
/* The same description evaluated POSITION BY POSITION - the element-wise counterpart of the step above: for p < len
 *     dst[p] = T[common][p_c] x sum_{m < nterms} (+/-) prod_{j < nfactors_m} T[factor_mj][p_mj]   (common == -1: the sum alone)
 * with table i read at p_i = (p + rot[i]) & (count_i - 1).  One op where a chain of blz_ntt_vec_op calls - one product or sum
 * each, every intermediate through a buffer - stood: the quotient numerator qL a + qR b + qM a b - qO c + qC on the 4n coset, a
 * custom gate that reads the next row, the random linear combination sum_j gamma^j f_j in front of an opening, the table
 * eq (Az Bz - Cz).  Arithmetic is over the handle's field and BY BUFFER POSITION: the bit-reversal flags and the coset shift play
 * no part, as for every op on the buffers.
 *   gate    blz_sum_gate as above: same layout, same limits, checked by the same code with the same messages.  A table index may
 *           repeat within a term and across terms, common may also be a factor, a table no term names is not read.
 *   tables  tables[0 .. ntables): operands as for blz_ntt_vec_op - a transform buffer, or `count` device words, a power of two
 *           with 1 <= count <= n, read periodically.  A one-word table is a scalar (a challenge power, a constant selector);
 *           four words carry 1 / Z_H on a 4x domain.  Messages name them tables[i].
 *   rot     ntables host values, copied by the call, or NULL for all zero.  Any 64-bit value: the index is taken modulo count_i
 *           in 64-bit arithmetic.  n - 1 reads the previous row, 4 on a 4n coset the next row of the n domain; the same words
 *           under two table indices with two rotations are Z and Z(wX) in one gate.
 *   dst     blz_ntt_vec_mle_fold's destination rule: a transform buffer, or the caller's device words (count a power of two,
 *           len <= count <= n).  1 <= len <= n, any value, not only powers of two.  EXACTLY len words are written; every other
 *           byte keeps its value (no zero fill).
 *   In place: dst may be a table, if that table starts where dst starts, holds at least len words and has rot[i] == 0 - a lane
 *           reads the position it owns before it writes it.  Every other meeting of a table's words with dst's len words is
 *           refused.  So dst <- dst + alpha a b is one op, dst a one-factor term of its own gate.
 *   Values: any 256-bit input word counts as its residue; every word written is canonical, little-endian.
 *   Cost ("Gate evaluation"; derived from the code): per position a table's word is read once per time a
 *   term or common names it (32 bytes from memory the first time, from cache after; a periodic table's from cache throughout)
 *   and 32 bytes are written.  Montgomery products per position: f for every term of f >= 2 factors (f - 1 for the product, 1
 *   for the constant R^f that takes the Montgomery powers off), none for a one-factor term, 2 for a common factor.  The PLONK
 *   gate above, five terms of 2, 2, 3, 2, 1 factors and no common factor: 9 products, 8 x 32 bytes read, 32 written; a linear
 *   combination of six: 12.
 *   Protocol: enqueued on the compute stream, the call returns; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms reports
 *   it, blz_ntt_reset drops it.  While it is in flight the buffer written may not be read, written or exchanged, a buffer that is
 *   only read may be read, and every transform, blz_ntt_set_coset and op on the buffers is refused.  Memory behind every device
 *   pointer stays valid, and operands unwritten, until blz_ntt_wait_result returns; the description and rot are copied.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing: a null handle (refused before any other argument is looked
 *   at), a null gate, dst or tables, every description error of blz_ntt_sumcheck_gate, len of 0 or above n, an op in flight, any
 *   operand error of blz_ntt_vec_op in a table or in dst, len above dst's count, a table that meets dst's len words without
 *   starting where dst starts, or that starts there with count < len or with a nonzero rotation. */
int blz_ntt_gate_eval(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* dst, const blz_vec_arg* tables, const uint64_t* rot,
                      uint64_t len);
/* Gate evaluation with LINEAR-FORM FACTORS - products of sums: a factor of a term, or the common factor, may be a linear form
 * over the tables instead of a table word.  For p < len
 *     dst[p] = C(p) x sum_{m < nterms} (+/-) prod_{j < nfactors_m} F_mj(p)                        (common == -1: the sum alone)
 *     F, C   = a table word T[i][p_i], p_i = (p + rot[i]) & (count_i - 1), or the value of a form
 *     L_k(p) = sum_{s < nsummands_k} (+/-) [ T[coef_s][p_coef] x ] T[table_s][p_table]
 * One op and no temporaries where blz_ntt_gate_eval needs one call per factor w + beta sigma + gamma into caller memory and one
 * more over the temporaries: the permutation argument's quotient term Z(wX) prod_j (w_j + beta sigma_j + gamma) -
 * Z prod_j (w_j + beta k_j X + gamma), the numerator and denominator columns behind Z, the logUp denominator
 * beta + sum_j gamma^j f_j, (Z - 1) L_1, a GKR layer add (x + y).  Arithmetic is over the handle's field and BY BUFFER POSITION:
 * the bit-reversal flags and the coset shift play no part, as for every op on the buffers.
 *   Layout (fixed; all fields little-endian, no padding):
 *     blz_lin_summand, 4 bytes:  0 coef (BLZ_LIN_NO_COEF = 0xFF: coefficient 1; else a table index) | 1 table (a table index) |
 *       2 negate (0: added, 1: subtracted) | 3 reserved, must be 0.
 *     blz_lin_form, 20 bytes:  0 nsummands (1 .. BLZ_LIN_MAX_SUMMANDS = 4) | 1 reserved[3], must be 0 | 4 summand[4], the first
 *       nsummands are read.
 *     terms are blz_gate_term unchanged: a factor byte below BLZ_LIN_FORM (0x80) is a table index, BLZ_LIN_FORM | k is form k.
 *     blz_lin_gate, 240 bytes:  0 ntables (1 .. BLZ_LIN_MAX_TABLES = 16) | 4 nterms (1 .. 8) | 8 common (-1, a table index, or
 *       BLZ_LIN_FORM | k) | 12 nforms (0 .. BLZ_LIN_MAX_FORMS = 8) | 16 term[8], the first nterms are read | 80 form[8], the
 *       first nforms are read.
 *   An index may repeat anywhere: within a term and across terms, within a form and across forms; a coefficient may be the table
 *   it multiplies (a square); a form may be named by several terms and as common; common may also be a factor.  A form that no
 *   term names is still checked but not evaluated; a table that nothing evaluated names is not read.  A constant is a one-word
 *   table with coef = BLZ_LIN_NO_COEF.  With nforms == 0 and ntables <= 12 the op writes the bytes blz_ntt_gate_eval writes.
 *   The three-wire permutation term takes 13 tables - Z twice (two rotations), a, b, c, sigma1 .. sigma3, X, beta, beta k1,
 *   beta k2, gamma -, six forms of three summands and two terms of four factors.
 *   tables  tables[0 .. ntables): operands as for blz_ntt_vec_op - a transform buffer, or `count` device words, a power of two
 *           with 1 <= count <= n, read periodically.  A one-word table is a scalar (a challenge power, a constant selector);
 *           four words carry 1 / Z_H on a 4x domain.  Messages name them tables[i].
 *   rot     ntables host values, copied by the call, or NULL for all zero: ONE rotation per table index, whatever names the
 *           index - a factor, a summand's table, a summand's coefficient.  Any 64-bit value: the index is taken modulo count_i
 *           in 64-bit arithmetic.  n - 1 reads the previous row, 4 on a 4n coset the next row of the n domain; the same words
 *           under two table indices with two rotations are Z and Z(wX) in one gate.
 *   dst     blz_ntt_vec_mle_fold's destination rule: a transform buffer, or the caller's device words (count a power of two,
 *           len <= count <= n).  1 <= len <= n, any value, not only powers of two.  EXACTLY len words are written; every other
 *           byte keeps its value (no zero fill).
 *   In place: dst may be a table, if that table starts where dst starts, holds at least len words and has rot[i] == 0 - a lane
 *           reads the position it owns before it writes it - whether the table is named as a factor, as a summand's table or
 *           as a summand's coefficient.  Every other meeting of a table's words with dst's len words is refused.
 *   Values: any 256-bit input word counts as its residue; every word written is canonical, little-endian.
 *   Cost ("Gate evaluation with linear forms"; derived from the code): per position a table's word is read
 *   once per time a term, a summand or common names it (32 bytes from memory the first time, from cache after; a periodic
 *   table's from cache throughout; a ONE-WORD coefficient is read once per block, not per position), a form is evaluated once
 *   per time it is named, and 32 bytes are written.  Montgomery products per position: per summand with a coefficient 1 if the
 *   coefficient is a one-word table, 2 if it is longer, none without a coefficient; f for every term of f >= 2 factors, none
 *   for a one-factor term; 2 for a common factor.  The permutation term above: 6 + 8 = 14 products, 9 x 32 bytes read (Z's second
 *   reading comes from cache), 32 written; the logUp denominator beta + gamma f1 + gamma^2 f2 + gamma^3 f3: 3.
 *   Protocol: enqueued on the compute stream, the call returns; blz_ntt_wait_result finishes it, blz_ntt_last_kernel_ms reports
 *   it, blz_ntt_reset drops it.  While it is in flight the buffer written may not be read, written or exchanged, a buffer that is
 *   only read may be read, and every transform, blz_ntt_set_coset and op on the buffers is refused.  Memory behind every device
 *   pointer stays valid, and operands unwritten, until blz_ntt_wait_result returns; the description and rot are copied.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing: a null handle (refused before any other argument is looked
 *   at), a null gate, dst or tables, ntables outside 1 .. 16, nterms outside 1 .. 8, nforms above 8, common below -1 or neither
 *   a table index below ntables nor BLZ_LIN_FORM | k with k below nforms, a term's nfactors outside 1 .. 4, a form's nsummands
 *   outside 1 .. 4, negate above 1 in a term or a summand, a factor that is neither a table index below ntables nor a form
 *   below nforms, a summand's table or coefficient (other than BLZ_LIN_NO_COEF) not below ntables, a nonzero reserved byte,
 *   len of 0 or above n, an op in flight, any operand error of blz_ntt_vec_op in a table or in dst, len above dst's count, a
 *   table that meets dst's len words without starting where dst starts, or that starts there with count < len or with a
 *   nonzero rotation. */
#define BLZ_LIN_MAX_TABLES   16
#define BLZ_LIN_MAX_FORMS     8
#define BLZ_LIN_MAX_SUMMANDS  4
#define BLZ_LIN_FORM       0x80   /* in a factor byte or in common: BLZ_LIN_FORM | k names form k */
#define BLZ_LIN_NO_COEF    0xFF   /* a summand's coef: the coefficient is 1 */
typedef struct blz_lin_summand {
    uint8_t coef;       /* BLZ_LIN_NO_COEF, or the table whose word multiplies the summand */
    uint8_t table;      /* a table index */
    uint8_t negate;     /* 0: the summand is added, 1: subtracted */
    uint8_t reserved;   /* must be 0 */
} blz_lin_summand;
typedef struct blz_lin_form {
    uint8_t nsummands;     /* 1 .. BLZ_LIN_MAX_SUMMANDS */
    uint8_t reserved[3];   /* must be 0 */
    blz_lin_summand summand[BLZ_LIN_MAX_SUMMANDS];   /* the first nsummands are read */
} blz_lin_form;
typedef struct blz_lin_gate {
    uint32_t ntables;   /* 1 .. BLZ_LIN_MAX_TABLES */
    uint32_t nterms;    /* 1 .. BLZ_GATE_MAX_TERMS */
    int32_t common;     /* -1: none; a table index; or BLZ_LIN_FORM | k */
    uint32_t nforms;    /* 0 .. BLZ_LIN_MAX_FORMS */
    blz_gate_term term[BLZ_GATE_MAX_TERMS];   /* the first nterms are read */
    blz_lin_form form[BLZ_LIN_MAX_FORMS];     /* the first nforms are read */
} blz_lin_gate;
int blz_ntt_gate_eval_lin(blz_ntt* h, const blz_lin_gate* gate, const blz_vec_arg* dst, const blz_vec_arg* tables,
                          const uint64_t* rot, uint64_t len);
/* The gate step of a ZEROCHECK, sum_p eq(tau, p) G(p) = 0 - blz_ntt_sumcheck_gate with the equality table taken out of the gate
 * and a SUMMED WEIGHT TABLE in its place (the eq-factor trick).  With top-variable pairing (p = sum x_i 2^i, round i binds
 * x_{m-1-i}; tau_i pairs with bit i as in blz_ntt_vec_mle_eq) the round polynomial factors:
 *     s_i(X) = c_i eq(tau_{m-1-i}, X) u_i(X),    u_i(X) = sum_p W_i[p] G(X, p),    eq(a, X) = a X + (1 - a)(1 - X),
 *     W_i = eq(tau_0 .. tau_{m-2-i}, .), 2^{m-1-i} words, the same for every X;   c_0 = 1, c_{i+1} = c_i eq(tau_{m-1-i}, r_i).
 * The op computes u_i: the degree of G, one below s_i, so one point fewer, and the weight multiplies the gate's sum once per
 * point.  The next weight is a SUM, not a fold by r - W_{i+1}[q] = W_i[q] + W_i[q + len / 4], since eq(tau, 0) + eq(tau, 1) = 1 -
 * and costs no product.  Reconstruction, on the host, O(points) per round: s_i(t) = c_i eq(tau_{m-1-i}, t) u_i(t) at the points
 * t = 0 .. points - 1, one more value of u_i by extrapolation (u_i has degree below points), then c_{i+1} from r_i.
 *   gate, tables   exactly blz_ntt_sumcheck_gate's: same struct, same limits, checked by the same code with the same messages.
 *           common stays available and counts as before.
 *   weight  required: the caller's device words, d_ptr != NULL, count a power of two in [1, n].  A transform buffer is refused.
 *           W_0 is blz_ntt_vec_mle_eq(point, m - 1) on the point buffer of the whole zerocheck: half the table.
 *   r == NULL - the first round: d_out[t] = sum_{p < len / 2} W[p & (count - 1)] G(.. lo_j + t (hi_j - lo_j) ..) for t < points,
 *     over the pairs (T[p], T[p + len / 2]).  Nothing is written besides d_out; periodic tables and a periodic weight are
 *     allowed.  len >= 2.
 *   r != NULL - bind, then round: every table is folded in place exactly as by blz_ntt_sumcheck_gate; W[q] <- W[q] + W[q + len / 4]
 *     for q < len / 4 - EXACTLY len / 4 weight words are written, every other byte of the weight keeps its value; then
 *       d_out[t] = sum_{q < len / 4} W[q] G(.., T_j[q] + t (T_j[q + len / 4] - T_j[q]), ..) over the folded tables and the new W.
 *     weight.count >= len / 2, len >= 4.
 *   1 <= points <= BLZ_GATE_MAX_POINTS.  points == 0 is refused: a bind alone has no weight, so a zerocheck's last op is
 *   blz_ntt_sumcheck_gate with points == 0.  An m-variable zerocheck is blz_ntt_vec_mle_eq(W, point, m - 1), one step without r at
 *   len = n, m - 1 steps with r, then that bind: m + 2 ops.
 *   Values: any 256-bit input word counts as its residue; every word written - table words, weight words and d_out - is
 *   canonical, little-endian.
 *   Cost ("Zerocheck step"; products derived from the code): blz_ntt_sumcheck_gate's count with `points`
 *   products for the weight in place of the 2 + points of a common eq table, at one point fewer: W (Az Bz - Cz) at 3 points is
 *   6 + 3 + 2 + 3 = 14 per quad where eq (Az Bz - Cz) at 4 is 18; the PLONK gate over its eight tables at 4 points 50 where nine
 *   tables at 5 cost 58.  The weight's traffic is len / 2 words read and len / 4 written where eq's is len read, len / 2 written.
 *   Protocol, in-flight rules and operand checks: blz_ntt_sumcheck_gate's, by the same code; everything is checked before
 *   anything is enqueued; one blz_ntt_wait_result.  Memory behind every pointer stays valid until it returns.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing, in this order: a null handle (refused before any other
 *   argument is looked at); a null gate, tables or weight; every description error of blz_ntt_sumcheck_gate; points == 0; a
 *   weight that names a buffer (d_ptr == NULL); then everything blz_ntt_sumcheck_gate refuses, in its order - points above 6, a
 *   null d_out, r naming a buffer or with count != 1, len not a power of two in [2, n] ([4, n] with r), an op in flight, any
 *   operand error of blz_ntt_vec_op in a table, in r or in the weight (messages name it `weight`), a bad d_out or one that
 *   overlaps a d_ptr operand - the weight's words, all `count` of them, included, in every mode; with r: a table with
 *   count < len, two tables whose first len words overlap, r inside the words a table receives, d_out inside the first len
 *   words of a table; and last, with r, the weight's own: count below len / 2, weight words [0, len / 2) meeting a table's first
 *   len words, r inside weight words [0, len / 4).  (d_out inside weight words [0, len / 2) is refused by the d_ptr-operand
 *   rule.) */
int blz_ntt_zerocheck_gate(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* tables, const blz_vec_arg* weight,
                           const blz_vec_arg* r, uint32_t points, uint64_t len, void* d_out);

/* ------------------------------------------------------------------ Poseidon octal Merkle tree (src/ingo_hash/poseidon_api.rs)
 *
 * THE HASH.  The reference does not define it: the permutation reaches the card as a CSV "instruction set" that does not ship.
 * As with the NTT's convention, it is the CALLER's: the word stream handed over at initialize carries the Poseidon instance.
 * Everything the reference does pin - call sequence, element FIFO, 11 elements per base node and arity 8 above
 * (tests/integration_poseidon.rs:109-116, 151-155), node count, the 64-byte record (poseidon_api.rs:42-71) - is kept exactly.
 *   Field: the scalar field of `field` (enum blz_curve); the reference's TEST_SCALAR is a BLS12-381 Fr element.
 *   Permutation of width t, textbook Poseidon, S-box x^5: R_F / 2 full rounds, R_P partial rounds, R_F / 2 full rounds; every
 *     round is: add the round's t constants -> S-box (all t elements in a full round, element 0 only in a partial one) ->
 *     multiply the state by the t x t MDS matrix M, new_i = sum_j M[i][j] s_j.  This dense form is the definition.
 *   Fixed-arity hash H_t(x_1 .. x_(t-1)): state = [tag_t, x_1, .., x_(t-1)], one permutation, digest = state[1].
 *   Tree of height h >= 1, layers 0 .. h - 1, layer l has 8^(h-1-l) nodes.
 *     BLZ_TREE_C (start layer 0): the input is a FIFO of 11 x 8^(h-1) elements; base node j = H_12(elements 11 j .. 11 j + 10);
 *       node i of layer l >= 1 = H_9(nodes 8 i .. 8 i + 7 of layer l - 1).  One record per node: (8^h - 1) / 7, 585 at h = 4.
 *     BLZ_TREE_D (start layer 1): the reference only writes the register.  THIS BUILD'S READING: the 8^(h-1) input elements ARE
 *       layer 0; records exist for layers 1 .. h - 1 only.
 *   Record, 64 bytes (PoseidonResult::parse_poseidon_hash_results): bytes 0-31 the digest, canonical little-endian; bytes 32-63 a
 *     256-bit little-endian word with hash_id (index inside the layer) in bits 0-29, layer_id in bits 30-39, zero above.
 *     Hence h <= 11; a larger height, or a tree whose buffers do not fit the device, is InvalidPrimitiveParam.
 *   Input elements >= r are taken as their residue (the NTT's rule).
 * PARITY WITH ANY OUTSIDE POSEIDON (Filecoin's neptune, circomlib ...) IS NOT PINNED: what is pinned is the definition above,
 * by an independent textbook implementation in tests/poseidon_ref.py.
 *
 * THE INSTRUCTION STREAM.  load_instructions (poseidon_api.rs:205-243) reads a CSV whose first line is a header and sends, per
 * record, the LAST column and then the SECOND-TO-LAST as 32-byte little-endian words.  This build gives that word stream a
 * meaning (the FPGA's microcode cannot be ours):
 *   magic ("BLZPOSEIDON01" as ASCII bytes = a little-endian integer: a CSV made for the card is refused, not misread), field,
 *   K, then K blocks of:  t, alpha (must be 5), R_F, R_P, tag_t, t (R_F + R_P) round constants in round order, t^2 MDS entries
 *   row-major;  an odd word count is padded with one zero word.
 * Checked at load: every word < r, R_F even, 2 <= t <= 16, no width twice, the block lengths add up, the widths the tree mode
 * needs are present (TreeC 9 and 12, TreeD 9).  Any failure is LoadFailed (poseidon_api.rs:100-103) and leaves the handle as it
 * was.  tools/poseidon_params.py writes such a CSV.
 *
 * ROUNDS.  The dense rounds above are the definition; by default the R_P partial rounds run in their optimised form, which gives
 * the same bytes.  With M = [[m00, v^T], [w, Mh]] (Mh: M without row 0 and column 0) partial round k = 1 .. R_P, j = R_P - k + 1,
 * multiplies by the sparse matrix [[m00, v^T Mh^-j], [Mh^(j-1) w, I]] (2t - 1 products instead of t^2) after adding the constants
 * diag(1, Mh^j) c_k, and the full round in front of them multiplies by diag(1, Mh^R_P) M.  A width admits this iff Mh is
 * invertible (R_P = 0: always).  The tables are derived ON THE DEVICE for the widths the tree mode hashes with, and self-checked:
 * a fixed batch of inputs (0, r - 1, words >= r among them) per width through both round forms, digests compared.  Equal: the
 * optimised rounds are in force.  A singular Mh or a differing digest: refused - the dense rounds run for every width; never an
 * error, the records are the same.  This preparation happens once per loaded instruction set, before the first tree's first launch
 * (outside blz_poseidon_last_kernel_ms) or when blz_poseidon_prepare_round_plan asks for it; never inside initialize. */
enum blz_tree_mode { BLZ_TREE_C = 0, BLZ_TREE_D = 1 };   /* src/ingo_hash/utils.rs:18-30 */

/* DriverClient::new + PoseidonClient::new(Hash::Poseidon, dclient) (poseidon_api.rs:77-79); field = enum blz_curve */
int blz_poseidon_new(int device_id, int field, blz_poseidon** out);
void blz_poseidon_free(blz_poseidon* h);
/* PoseidonClient::loaded_binary_parameters (poseidon_api.rs:81-94): [image_id, image_parameters]; word 1 decodes with
 * PoseidonImageParametrs (:256-271): is_stub 0, number_of_cores = min(compute units, 255) */
int blz_poseidon_loaded_binary_parameters(blz_poseidon* h, uint32_t out[2]);
/* PoseidonClient::initialize(PoseidonInitializeParameters{tree_height, tree_mode, instruction_path}) (poseidon_api.rs:96-111):
 * reset, load the instruction set, height, start layer.  Allocates the tree's buffers: inputs of one tree + every layer (32 B
 * per node) + records (64 B per node); TreeC at h = 8 holds 738 MB of input.  A call that passes the checks (arguments, stream, memory
 * estimate) and then fails in an allocation or a transfer leaves the handle UNINITIALISED: the earlier tree's buffers are gone by then. */
int blz_poseidon_initialize(blz_poseidon* h, uint32_t tree_height, int tree_mode, const char* instruction_path);
/* The load-time checks alone, host side, no device (like blz_msm_plan): out (nullable) = {blocks, bit mask of the widths,
 * 0, words consumed}.  Word 2 is reserved: whether the widths admit the optimised partial rounds takes field arithmetic, which
 * the host side does not have - blz_poseidon_prepare_round_plan / blz_poseidon_info give that answer. */
int blz_poseidon_check_words(int field, int tree_mode, const uint8_t* words, size_t len, uint32_t out[4]);
/* initialize with the word stream from memory (len bytes = len / 32 words) */
int blz_poseidon_initialize_words(blz_poseidon* h, uint32_t tree_height, int tree_mode, const uint8_t* words, size_t len);
/* PoseidonClient::set_data(&[u8]) (poseidon_api.rs:117-122): elements into the FIFO.  len a multiple of 32: len / 32 elements;
 * 0 < len < 32 (host memory only): ONE element, zero-extended - the reference's tests write 4-byte and to_bytes_le() buffers, one
 * element per call, and test_sanity_check expects the element counter to go up by one per call; anything else, or a call before
 * initialize, is InvalidPrimitiveParam.  Blocking like the other set_datas (the buffer is free on return).
 * The FIFO is a stream: nodes are hashed as soon as a worthwhile batch (1024) of complete inputs exists, and always when the tree's
 * last element arrives; an upper node when its eight children are.  Records become pending in an unspecified order, every node
 * exactly once and never before its children.  After a tree's last element the next element starts the next tree, ids from
 * zero (the card runs continuously); records of the finished tree that nobody has read stay pending.  A tree whose whole input
 * arrives in one call takes ONE kernel launch per layer. */
int blz_poseidon_set_data(blz_poseidon* h, const uint8_t* data, size_t len);
int blz_poseidon_set_data_device(blz_poseidon* h, const void* d_data, size_t len);
/* PoseidonClient::wait_result is todo!() in the reference (poseidon_api.rs:124-126).  Here: when it returns, every node whose
 * inputs have arrived has been hashed and its record is pending.  Bounded (BLAZE_WAIT_TIMEOUT_MS, reset-only rule as above). */
int blz_poseidon_wait_result(blz_poseidon* h);
/* PoseidonClient::get_num_of_pending_results (poseidon_api.rs:156-161) */
int blz_poseidon_num_pending_results(blz_poseidon* h, uint32_t* out);
/* PoseidonClient::get_raw_results(n) (poseidon_api.rs:191-196): pops n (<= pending) records, 64 n bytes */
int blz_poseidon_raw_results(blz_poseidon* h, uint32_t n, uint8_t* out, size_t cap);
/* PoseidonClient::result(Some(expected)) (poseidon_api.rs:128-145): pops up to `expected` records, *n says how many.  Bounded where
 * the reference spins: everything the elements fed so far can produce is hashed first; if that is fewer than `expected` records
 * the call returns them (the reference would poll for ever). */
int blz_poseidon_result(blz_poseidon* h, uint32_t expected, uint8_t* out, size_t cap, uint32_t* n);
/* every record of the finished tree in (layer, id) order, device to device; pops them.  Needs a finished tree none of whose records
 * has been read and no older records pending.  No reference counterpart (see blz_msm_set_data_device). */
int blz_poseidon_tree_device(blz_poseidon* h, void* d_out, size_t cap);
/* out = {elements accepted since initialize, modulo 2^32 (LAST_ELEMENT_ID_SENT_TO_RING, poseidon_api.rs:149-154: + 1 per element),
 * hash_id of the last record handed to the host (LAST_HASH_ID_SENT_TO_HOST, :198-203), its layer_id, elements of the current
 * tree no hash has consumed yet} */
int blz_poseidon_counters(blz_poseidon* h, uint32_t out[4]);
/* out = {device bytes held (the derived tables included), 1 if the optimised partial rounds are in force (setting 1 and self-check
 * equal), state of their self-check for the loaded instruction set (0 not run yet, 1 equal, 2 refused), bit mask of the widths loaded} */
int blz_poseidon_info(blz_poseidon* h, uint64_t out[4]);
/* 1 (default): optimised partial rounds if their self-check holds; 0: dense always, at once.  Back to 1 reuses the tables already
 * derived.  The setting survives initialize and reset; initialize discards the tables and the self-check state, reset keeps them. */
int blz_poseidon_set_round_plan(blz_poseidon* h, int enable);
/* Derive and self-check the optimised partial rounds NOW instead of under the first tree (cf. blz_msm_prepare_window_table).
 * out (nullable) = {in force, self-check state} as blz_poseidon_info reports them.  With the setting at 0 it does nothing and
 * returns OK.  Null handle: InvalidPrimitiveParam; before initialize: InvalidPrimitiveParam; wedged handle: Unknown.  Blocking,
 * bounded (BLAZE_WAIT_TIMEOUT_MS).  A refusal (state 2) is not an error. */
int blz_poseidon_prepare_round_plan(blz_poseidon* h, uint32_t out[2]);
/* device time from the first layer launch of the last finished tree to its last, ms */
int blz_poseidon_last_kernel_ms(blz_poseidon* h, float* out);
/* the HIP stream the layer kernels run on; see blz_msm_stream */
int blz_poseidon_stream(blz_poseidon* h, void** hip_stream, int* device_id);
/* DriverClient::reset (dclient.rs:88-93): drops the partial tree and every pending record; the instruction set, the height and
 * the mode stay */
int blz_poseidon_reset(blz_poseidon* h);

/* ------------------------------------------------------------------ Fiat-Shamir transcript and the one-call sumcheck prover
 *
 * Two ops on a blz_ntt handle.  They stand here, behind the step ops they chain (blz_ntt_sumcheck_gate, blz_ntt_zerocheck_gate),
 * because with them the host leaves the loop: every op above is ONE step, and between two steps a prover had to wait, download
 * the round polynomial, hash it into a challenge and upload that - about 52 us a round at any table size (DESIGN.md section 4,
 * "One-call prover").  r was made a device word so that a transcript could be added without touching the steps; this is it.
 *
 * THE TRANSCRIPT STEP.  The hash is SHA3-256 (FIPS 202): a byte-oriented hash costs a few microseconds on one wave where a lone
 * Poseidon permutation costs more than the round trip it would replace.  Python's hashlib.sha3_256 reproduces it.
 *   d_state is one 32-byte device word, 16-byte aligned.  It is read and written.
 *   digest = SHA3-256(state || w_0 || ... || w_{count-1}).
 *   The w_i are the first `count` 32-byte words of `words`, exactly as stored.  Nothing is reduced.  The ops write canonical
 *   words anyway.
 *   0 <= count <= 32.  `words` may be NULL when count is 0.
 *   `words` is a transform buffer or device words, as for any operand (blz_ntt_vec_op's rules; it holds at least `count` words).
 *   The new state is the digest.
 *   The challenge written to d_r is the digest read as a little-endian 256-bit integer, with every bit from bit
 *   bitlen(modulus) - 1 upward cleared.  That keeps 252 bits on BLS12-377, 254 on BLS12-381 and 253 on BN254.
 *   Because of the masking the challenge is uniform and always canonical.  d_r is nullable; NULL means absorb only.
 *   The protocol is every op's: checked first, enqueued, finished by blz_ntt_wait_result, timed by blz_ntt_last_kernel_ms.
 *   d_state and d_r must not overlap each other or the words read.
 *   A buffer named by `words` is read-only while the op is in flight; no transform buffer is written.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing, in this order: a null handle (refused before any other
 *   argument is looked at), a null d_state, count above 32, a null `words` with count > 0, an op in flight, any operand error of
 *   blz_ntt_vec_op in `words`, `words` holding fewer than `count` words, a d_state or d_r that is misaligned, not device memory of
 *   the handle's device or running past its allocation, d_r overlapping d_state, d_state or d_r inside the words absorbed. */
int blz_ntt_fs_challenge(blz_ntt* h, void* d_state, const blz_vec_arg* words, uint32_t count, void* d_r);
/* THE ONE-CALL PROVER.  A whole m-variable sumcheck, m = log2 len >= 1, enqueued by ONE call with no host wait inside: the m + 2
 * step ops and the m transcript steps between them, on the handle's compute stream, each behind the one before.
 *   weight == NULL proves sum_p G(p) with blz_ntt_sumcheck_gate's steps; otherwise sum_p W[p] G(p) with blz_ntt_zerocheck_gate's -
 *   the weight is len / 2 device words, and the eq factor stays with the caller exactly as for the single step.
 *   gate, tables: blz_ntt_sumcheck_gate's, checked by the same code with the same messages.  1 <= points <= BLZ_GATE_MAX_POINTS.
 *   The chain:  1. the round alone at len writes d_rounds[0 .. points);
 *               2. for i = 0 .. m - 1 the transcript step absorbs row i of d_rounds (points words) and writes d_challenges[i];
 *               3. for i < m - 1 the step with r = d_challenges[i] at live length len >> i follows and writes row i + 1;
 *               4. last comes the bind alone - blz_ntt_sumcheck_gate with points == 0 at length 2 - with d_challenges[m - 1].
 *   Afterwards word 0 of every table is that table at the challenges, top variable first; d_rounds holds m x points words,
 *   d_challenges m words, and d_state the state after the last absorb: a caller chains the next sumcheck, or derives batching
 *   challenges, with blz_ntt_fs_challenge.  The final table words are NOT absorbed by the call.
 *   Bytes written are exactly the bytes the equivalent sequence of single ops writes and no others: at most len / 2 words of
 *   each table, at most len / 4 of the weight, and the three outputs.
 *   Everything is checked before the first launch.  The bind rules hold from the start - no periodic table, no two tables
 *   meeting in their first len words; the weight's rules are blz_ntt_zerocheck_gate's; the three outputs lie off every table's
 *   first len words, off the weight's words and off each other.
 *   Protocol: one blz_ntt_wait_result finishes the chain and blz_ntt_last_kernel_ms then spans it; blz_ntt_reset drops it.  While
 *   it runs, every transform buffer that is a table is a buffer being written (both may be), and no op starts.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing, in this order: a null handle (refused before any other
 *   argument is looked at); a null gate, tables, d_state, d_rounds or d_challenges; every description error of
 *   blz_ntt_sumcheck_gate; points outside 1 .. 6; a weight that names a buffer; len not a power of two in [2, n]; an op in flight;
 *   any operand error of blz_ntt_vec_op in a table or in the weight; a table with count < len; two tables whose first len words
 *   meet; a weight below len / 2 words or whose first len / 2 words meet a table's first len; then per output, in the order
 *   d_state, d_rounds, d_challenges: misaligned, not device memory of the handle's device or running past its allocation, inside
 *   a table's first len words, inside the weight's words, overlapping an earlier output. */
int blz_ntt_sumcheck_prove(blz_ntt* h, const blz_sum_gate* gate, const blz_vec_arg* tables, const blz_vec_arg* weight, uint32_t points,
                           uint64_t len, void* d_state, void* d_rounds, void* d_challenges);
/* THE ONE-CALL GKR PROVER.  The GKR grand product over a product tree, enqueued by ONE call with no host wait inside: the argument
 * blz_ntt_mle_tree and blz_ntt_sumcheck_prove were built for.  A grand product over len = 2^m leaves is m layers and
 * m (m - 1) / 2 sumcheck rounds, almost all of them over tables of a few hundred words; without BLZ_GKR_UNFUSED every round at a
 * live length of 512 and below - all of them for m <= 10 - runs inside one block that keeps the layer's tables in LDS
 * ("One-call GKR").
 *   op: BLZ_TREE_PROD.  BLZ_TREE_FRAC is refused by name: it is not built here (blz_ntt_gkr_prove_frac takes fraction trees).
 *   flags: 0, or BLZ_GKR_UNFUSED: the chain of the existing step launches alone.  Both write the same bytes to the four outputs.
 *   tree: a BLZ_TREE_PROD tree over the len leaves `a` with the default pairing, exactly as blz_ntt_mle_tree(dst = tree, a) leaves
 *   it: layer k, 1 <= k <= m, holds len / 2^k words at word len - len / 2^(k-1); layer 0 is `a`.  Both are operands like any
 *   other - a transform buffer or device words, at least len - 1 and len of them, not periodic - and may be the handle's two
 *   buffers.  d_weight: max(len / 4, 1) device words, the scratch for the weight.  d_state: the transcript, one word.
 *   THE LAYERS are taken from the root down, j = 0 .. m - 1.  lo and hi of layer j are the two halves of layer m - 1 - j of the
 *   tree (of `a` for j = m - 1), 2^j words each.
 *   OUTPUTS, device words:
 *     d_rounds  3 m (m - 1) / 2 words; round i < j of layer j is the three words at word 3 (j (j - 1) / 2 + i);
 *     d_points  m (m + 1) / 2 words; row j is j + 1 words at word j (j + 1) / 2;
 *     d_claims  2 m words; row j is (lo_f, hi_f) at words 2 j and 2 j + 1.
 *   LAYER j >= 1: tau is row j - 1 of d_points (tau_i paired with bit i, as blz_ntt_vec_mle_eq reads a point); the weight is
 *   W = eq(tau_0 .. tau_{j-2}), 2^(j-1) words; the sumcheck is the one blz_ntt_sumcheck_prove enqueues under a weight over the
 *   tables [lo, hi] and the gate + lo hi at 3 points and live length 2^j, except that round i's three words land at the place
 *   above and its challenge at word j - 1 - i of row j of d_points: the steps bind the top variable first, so the row is left in
 *   bit order and is the next layer's point as it stands.  The eq factor stays out of the gate as for blz_ntt_zerocheck_gate:
 *   the words of d_rounds are u_i(0), u_i(1), u_i(2) with s_i(X) = c eq(tau_{j-1-i}, X) u_i(X).
 *   EVERY LAYER j >= 0, behind its sumcheck (j = 0 has none): lo[0] and hi[0] - the tables at the challenges; for j = 0 the
 *   root's own pair - are copied to row j of d_claims, one transcript step absorbs those two words as stored, and its challenge
 *   rho_j lands at word j of row j of d_points.  lo is the half with the top bit clear: rho_j is the top variable of the layer
 *   below, whose claim is lo_f + rho_j (hi_f - lo_f).  After the last layer that claim is the multilinear extension of the
 *   leaves at row m - 1 of d_points.  blaze_amd/gkr.py verify_product is the verifier.
 *   d_state is read at the start and left at the state after the last step.  The root is NOT absorbed by the call: a caller who
 *   wants it in the transcript absorbs it with blz_ntt_fs_challenge first.
 *   BYTES WRITTEN.  The tree is consumed.  Of each layer's halves, and of a's, only the words the chain of single ops writes may
 *   be touched - the first half of lo and the first half of hi - and their contents afterwards are unspecified (the fused path
 *   leaves the layers of 512 words and below as they were).  Every other byte of tree and a keeps its value: the upper half of
 *   each half-layer, and the tree's word beyond len - 2.  Of d_weight at most len / 4 words are written: the equality table of the
 *   largest layer, whose first len / 8 the steps then sum into.
 *   Protocol: one blz_ntt_wait_result finishes the op and blz_ntt_last_kernel_ms then spans it; blz_ntt_reset drops it.  While
 *   it runs, a transform buffer that tree or a names is a buffer being written, and no op starts.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing, in this order: a null handle (refused before any other
 *   argument is looked at); BLZ_TREE_FRAC or an unknown op; unknown flag bits; a null tree, a, d_weight, d_state, d_rounds,
 *   d_points or d_claims, each named; len not a power of two in [2, n]; an op in flight; any operand error of blz_ntt_vec_op in
 *   tree or a, a tree below len - 1 words, leaves below len; then per pointer, in the order d_weight, d_state, d_rounds, d_points,
 *   d_claims: misaligned, not device memory of the handle's device or running past its allocation; then the overlaps, each message
 *   naming both sides: a's len words against the tree's len - 1, the weight's max(len / 4, 1) against both, and each output
 *   against all of those and against the outputs before it. */
#define BLZ_GKR_UNFUSED 1u   /* the chain of existing launches only: the A/B side of the fused kernel */
int blz_ntt_gkr_prove(blz_ntt* h, uint32_t op, uint32_t flags, const blz_vec_arg* tree, const blz_vec_arg* a, uint64_t len, void* d_weight,
                      void* d_state, void* d_rounds, void* d_points, void* d_claims);
/* THE ONE-CALL FRACTION GKR PROVER.  The GKR argument over a FRACTION tree (logUp-GKR, memory checking with fractions), enqueued
 * by ONE call with no host wait inside: blz_ntt_gkr_prove over four tables a layer.  A sum of len = 2^m fractions a_p / a_q is m
 * layers and m (m - 1) / 2 sumcheck rounds; without BLZ_GKR_UNFUSED every round at a live length of 256 and below - all of them
 * for m <= 9 - runs inside one block that keeps the layer's four tables in LDS ("One-call fraction GKR").
 *   flags: 0, or BLZ_GKR_UNFUSED: the chain of the existing launches alone.  Both write the same bytes to the five outputs.
 *   tree_p, tree_q: the numerator and the denominator tree, exactly as blz_ntt_mle_tree(BLZ_TREE_FRAC, dst = tree_p, dst_q =
 *   tree_q, a_p, a_q, len) left them with the default pairing: layer k, 1 <= k <= m, holds len / 2^k words at word len - len /
 *   2^(k-1) of each; layer 0 is the leaves a_p, a_q.  2 <= len <= n.  All four are operands like any other - a transform buffer
 *   or device words, at least len - 1 (a tree) and len (leaves) of them - and none is periodic: a one-word numerator 1 is
 *   expanded by the caller first (blz_ntt_vec_gather), because the leaves are folded in place.  At most two of the four can name
 *   a transform buffer.  d_weight: max(len / 4, 1) device words, the scratch for the weight, used as in blz_ntt_gkr_prove.
 *   d_state: the transcript, one word.
 *   THE LAYERS are taken from the root down, j = 0 .. m - 1.  P_lo, P_hi are the two halves of layer m - 1 - j of tree_p (of a_p
 *   for j = m - 1), Q_lo, Q_hi the same of tree_q / a_q, 2^j words each; lo is the half with the top bit clear.
 *   OUTPUTS, device words:
 *     d_rounds   3 m (m - 1) / 2 words; round i < j of layer j is the three words u_i(0), u_i(1), u_i(2) at word
 *                3 (j (j - 1) / 2 + i);
 *     d_points   m (m + 1) / 2 words; row j is j + 1 words at word j (j + 1) / 2;
 *     d_claims   4 m words; row j is (P_lo_f, P_hi_f, Q_lo_f, Q_hi_f) at word 4 j;
 *     d_lambdas  m words; word j >= 1 is lambda_j.  Word 0 is never written and keeps its bytes.
 *   LAYER j >= 1, in order.  Its claims from the layer above are P(tau), Q(tau) with tau row j - 1 of d_points.
 *     1. One transcript step with count 0 (digest = SHA3-256(state)) writes the batching challenge lambda_j to word j of d_lambdas.
 *        The layer proves  P(tau) + lambda_j Q(tau) = sum_p eq(tau, p) [ P_lo Q_hi + P_hi Q_lo + lambda_j Q_lo Q_hi ]
 *                                                  = sum_p eq(tau, p) [ P_lo Q_hi + Q_lo T ],  T = P_hi + lambda_j Q_hi.
 *     2. T is written over the 2^j words of P_hi, every word canonical.  T is linear in the tables, so binding a variable
 *        commutes with it, and the gate needs no scalar.
 *     3. W = eq(tau_0 .. tau_{j-2}), 2^(j-1) words, is built (tau_i paired with bit i, as blz_ntt_vec_mle_eq reads a point).
 *     4. The sumcheck blz_ntt_sumcheck_prove enqueues under a weight, over the tables [P_lo, T, Q_lo, Q_hi] and the gate
 *        + [0, 3] + [2, 1] at 3 points and live length 2^j, except that round i's three words land at the place above and its
 *        challenge at word j - 1 - i of row j of d_points: the steps bind the top variable first, so the row is left in bit order.
 *        The eq factor stays out of the gate as for blz_ntt_zerocheck_gate: s_i(X) = c eq(tau_{j-1-i}, X) u_i(X).
 *     5. The claims are P_lo_f, T_f - lambda_j Q_hi_f (canonical), Q_lo_f and Q_hi_f: the four tables at the challenges.
 *   LAYER 0 has no lambda and no sumcheck: its claims are the root's four children copied as stored.
 *   EVERY LAYER j >= 0, behind its claims: ONE transcript step absorbs the four claim words as stored - 160 bytes with the state,
 *   two blocks of SHA3-256's 136-byte rate - and its challenge rho_j lands at word j of row j of d_points.  The next layer's
 *   claims are P = P_lo_f + rho_j (P_hi_f - P_lo_f) and the same for Q.  After the last layer they are the multilinear extensions
 *   of a_p and of a_q at row m - 1 of d_points.  The verifier holds a layer's end to
 *   c (P_lo_f Q_hi_f + P_hi_f Q_lo_f + lambda_j Q_lo_f Q_hi_f) = claim; blaze_amd/gkr.py verify_fraction is that verifier.
 *   d_state is read at the start and left at the state after the last step.  The roots are NOT absorbed by the call: a caller who
 *   wants them in the transcript absorbs them with blz_ntt_fs_challenge first.
 *   BYTES WRITTEN.  The trees and the leaves are consumed.  Of each layer of tree_p / a_p only the whole hi half (T) and the
 *   first half of the lo half may be touched; of tree_q / a_q only the first half of each half.  Their contents afterwards are
 *   unspecified (the fused path leaves the layers it takes whole, 256 words a table and below, untouched).  Every other byte
 *   keeps its value, word len - 2 (the root) and everything behind it included.  Of d_weight at most len / 4 words are written,
 *   of d_lambdas m - 1.
 *   Protocol: blz_ntt_gkr_prove's.  One blz_ntt_wait_result finishes the op and blz_ntt_last_kernel_ms then spans it;
 *   blz_ntt_reset drops it.  While it runs, a transform buffer that any of the four operands names is a buffer being written, and
 *   no op starts.
 *   BLZ_ERR_INVALID_PARAM, changing nothing and enqueueing nothing, in this order: a null handle (refused before any other
 *   argument is looked at); unknown flag bits; a null tree_p, tree_q, a_p, a_q, d_weight, d_state, d_rounds, d_points, d_claims
 *   or d_lambdas, each named; len not a power of two in [2, n]; an op in flight; any operand error of blz_ntt_vec_op in the four
 *   operands; a tree below len - 1 words, leaves below len; then per pointer, in the order d_weight, d_state, d_rounds, d_points,
 *   d_claims, d_lambdas: misaligned, not device memory of the handle's device or running past its allocation; then the overlaps,
 *   each message naming both sides: every range against every range before it, in the order tree_p, tree_q (len - 1 words
 *   each), a_p, a_q (len each), the weight's max(len / 4, 1), then the five outputs. */
int blz_ntt_gkr_prove_frac(blz_ntt* h, uint32_t flags, const blz_vec_arg* tree_p, const blz_vec_arg* tree_q, const blz_vec_arg* a_p,
                           const blz_vec_arg* a_q, uint64_t len, void* d_weight, void* d_state, void* d_rounds, void* d_points, void* d_claims,
                           void* d_lambdas);

/* ------------------------------------------------------------------ device / host memory helpers */

/* Device memory owned by the library (hosts without a tensor library of their own; bench.py and the tests use these). */
int blz_device_malloc(int device_id, size_t bytes, void** out);
int blz_device_free(int device_id, void* p);
/* Host memory the runtime can DMA from / to without staging (page-locked, mapped for `device_id`): copies out of and into such
 * buffers are truly asynchronous, which is what lets blz_ntt_exchange keep both directions of the link busy from one thread.
 * Any pointer works everywhere (pageable memory is staged by the runtime); these are for hosts that own their I/O vectors. */
int blz_host_malloc(int device_id, size_t bytes, void** out);
int blz_host_free(void* p);
int blz_memcpy_h2d(int device_id, void* d_dst, const void* src, size_t bytes);
int blz_memcpy_d2h(int device_id, void* dst, const void* d_src, size_t bytes);
#ifdef __cplusplus
}
#endif
#endif /* BLAZE_HIP_H */
