// engine.hip - creates the engine object of libaz_mcts.so (az_mcts, engine_internal.h) and implements
// create/destroy/seed/config, capacity and instrumentation of the C ABI of include/az_mcts.h.
#include "engine_internal.h"

thread_local std::string az::host::g_last_error;

namespace {
constexpr int64_t kInitialSlots = 4096;

az_mcts *create_engine(int game, int n_envs, int device)
{
    if (!known_game(game)) throw AzError(AZ_ERR_ARG, "unknown game id");
    if (n_envs <= 0) throw AzError(AZ_ERR_ARG, "n_envs must be positive");
    int count = 0;
    const hipError_t dev_err = hipGetDeviceCount(&count);
    if (dev_err != hipSuccess || count <= 0)
        throw AzError(AZ_ERR_DEVICE, std::string("no HIP device available: the search engine runs on the GPU only (hipGetDeviceCount: ") +
                                         hipGetErrorString(dev_err) + ", " + std::to_string(count) + " devices)");
    if (device >= 0) HIP_OK(hipSetDevice(device));
    auto *m = new az_mcts();
    try {
        HIP_OK(hipGetDevice(&m->device));
        m->game = game;
        m->geo = geo_of(game);
        m->vl_leaf.max_path = m->plain_leaf.max_path = m->geo.max_path;
        m->B = n_envs;
        m->cfg.c_init = 1.25f; m->cfg.c_base = 19652.0f; m->cfg.dirichlet_alpha = 0.3f;
        m->cfg.noise_epsilon = 0.25f; m->cfg.fpu_reduction = 0.4f; m->cfg.mlh_slope = 0.0f;
        m->cfg.mlh_cap = 0.2f; m->cfg.score_utility_factor = 0.0f; m->cfg.score_scale = 8.0f;
        m->cfg.value_decay = 1.0f; m->cfg.use_symmetry = 1; m->cfg.vl_count = 1;
        m->S = kInitialSlots;
        m->hot.ensure(static_cast<size_t>(n_envs) * 2 * m->S);
        m->cold.ensure(static_cast<size_t>(n_envs) * 2 * m->S);
        m->root.ensure(n_envs); m->used.ensure(n_envs); m->half.ensure(n_envs, true);
        m->max_live.ensure(1, true);
        {
            int *ring = nullptr;
            HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&ring), 8 * sizeof(int), hipHostMallocDefault));
            for (int i = 0; i < 8; ++i) ring[i] = -1;
            m->live_ring = ring;
        }
        m->r_bb0.ensure(n_envs, true); m->r_bb1.ensure(n_envs, true);
        m->r_turn.ensure(n_envs, true); m->r_last.ensure(n_envs, true);
        m->counters.ensure(az::CNT_N * az::CNT_STRIPES, true);
        m->err.ensure(1, true);
        HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&m->err_host), sizeof(int), hipHostMallocDefault));
        *m->err_host = 0;
        m->call_ctr.ensure(1, true);
        m->plain_leaf.ensure(n_envs);
        m->pending_reset.assign(n_envs, 0);
        m->stash_root_nv.assign(n_envs, 0);
        az::launch_init_trees(m->arena(), nullptr);
        HIP_OK(hipDeviceSynchronize());
    } catch (...) {
        delete m;
        throw;
    }
    return m;
}
}  // namespace

// ====================================================================== C ABI

extern "C" {

const char *az_last_error(void) { return g_last_error.c_str(); }

int az_game_action_size(int game) { return known_game(game) ? geo_of(game).actions : -1; }
int az_game_board_size(int game) { return known_game(game) ? geo_of(game).cells : -1; }
int az_game_board_rows(int game) { return known_game(game) ? geo_of(game).rows : -1; }
int az_game_board_cols(int game) { return known_game(game) ? geo_of(game).cols : -1; }

int az_mcts_create(int game, int n_envs, int device, az_mcts **out)
{
    return guarded([&] {
        require(out != nullptr, "out is null");
        *out = create_engine(game, n_envs, device);
    });
}

void az_mcts_destroy(az_mcts *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    delete m;
}

az_search_config *az_mcts_config(az_mcts *m) { return &m->cfg; }
int az_mcts_num_envs(const az_mcts *m) { return m->B; }

int az_mcts_set_seed(az_mcts *m, int seed)
{
    return guarded([&] {
        if (seed < 0) {                       // BatchedMCTS.h:73-76
            m->rng.seed_random();
            m->dev_seed = (static_cast<uint64_t>(m->rng.next()) << 32) | m->rng.next();
        } else {                              // thread 0: seed + 0*10007 (BatchedMCTS.h:79-81)
            m->rng.seed(static_cast<uint32_t>(seed));
            m->dev_seed = static_cast<uint64_t>(static_cast<uint32_t>(seed)) * 0x9E3779B97F4A7C15ull + 1;
        }
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipMemset(m->call_ctr.p, 0, sizeof(uint64_t)));
    });
}

int az_mcts_reset_env(az_mcts *m, int env)
{
    if (env >= 0 && env < m->B) {             // silently ignores out-of-range (BatchedMCTS.h:95)
        m->pending_reset[env] = 1;
        m->any_pending_reset = true;
    }
    return AZ_OK;
}

// ---------------------------------------------------------------- capacity / instrumentation

int az_mcts_reserve(az_mcts *m, int64_t slots_per_tree)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        if (slots_per_tree > m->S) m->grow(slots_per_tree);
    });
}

int64_t az_mcts_capacity(const az_mcts *m) { return m->S; }
int64_t az_mcts_epoch(const az_mcts *m) { return m->epoch; }

int az_c4_dev_step(uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, const int32_t *actions,
                   uint8_t *done, int32_t *winner, int64_t n, int reset_finished, void *stream)
{
    return guarded([&] {
        require(n >= 0, "az_c4_dev_step: negative size");
        if (n == 0) return;
        az::launch_game_step(AZ_GAME_CONNECT4, bb_p1, bb_p2, turns, nullptr, actions, done, winner, n, reset_finished != 0,
                             static_cast<hipStream_t>(stream));
    });
}

int az_game_dev_step(int game, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, int32_t *aux, const int32_t *actions,
                     uint8_t *done, int32_t *winner, int64_t n, int reset_finished, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_game_dev_step: unknown game");
        require(n >= 0, "az_game_dev_step: negative size");
        if (n == 0) return;
        az::launch_game_step(game, bb_p1, bb_p2, turns, aux, actions, done, winner, n, reset_finished != 0,
                             static_cast<hipStream_t>(stream));
    });
}

int az_game_dev_valid_mask(int game, const uint64_t *bb_p1, const uint64_t *bb_p2, const int32_t *turns,
                           const int32_t *aux, uint8_t *mask, int64_t n, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_game_dev_valid_mask: unknown game");
        require(n >= 0, "az_game_dev_valid_mask: negative size");
        if (n == 0) return;
        az::launch_game_valid_mask(game, bb_p1, bb_p2, turns, aux, mask, n, static_cast<hipStream_t>(stream));
    });
}

int az_game_dev_pick(int game, const int32_t *counts, const float *q, const int32_t *ply, const uint8_t *dead,
                     int32_t *actions, int64_t n, int temp_decay_moves, int hot_early, int hot_late, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_game_dev_pick: unknown game");
        require(n >= 0 && n <= INT32_MAX, "az_game_dev_pick: size out of range");
        require(counts && q && ply && actions, "az_game_dev_pick: null array");
        if (n == 0) return;
        az::launch_ply_pick(game, counts, q, ply, dead, actions, static_cast<int>(n), temp_decay_moves, hot_early != 0,
                            hot_late != 0, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_ply_advance(az_mcts *m, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, int32_t *aux,
                            const int32_t *actions, uint8_t *done, int32_t *winner, int32_t *ply, uint8_t *dead,
                            int64_t *totals, int refill, void *stream)
{
    return guarded([&] {
        require(bb_p1 && bb_p2 && turns && aux && actions && done && winner && ply && dead && totals,
                "az_mcts_dev_ply_advance: null array");
        az::launch_ply_advance(m->game, m->arena(), bb_p1, bb_p2, turns, aux, actions, done, winner, ply, dead, totals,
                               refill != 0, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_max_used(az_mcts *m, int64_t *out)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        m->flush_resets(nullptr);
        HIP_OK(hipDeviceSynchronize());
        *out = m->true_max_used();
        m->used_bound = *out;
    });
}

int az_mcts_counters(az_mcts *m, int64_t out[AZ_NUM_COUNTERS])
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        unsigned long long h[az::CNT_N * az::CNT_STRIPES];
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(h, m->counters.p, sizeof h, hipMemcpyDeviceToHost));
        for (int i = 0; i < az::CNT_N; ++i) {
            unsigned long long sum = 0;
            for (int st = 0; st < az::CNT_STRIPES; ++st) sum += h[st * az::CNT_N + i];
            out[i] = static_cast<int64_t>(sum);
        }
        out[az::CNT_SELECT_LAUNCHES] = m->select_launches;
        out[az::CNT_BACKPROP_LAUNCHES] = m->backprop_launches;
        m->check_device_error();
    });
}

int az_mcts_counters_reset(az_mcts *m)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemset(m->counters.p, 0, sizeof(unsigned long long) * az::CNT_N * az::CNT_STRIPES));
        m->select_launches = m->backprop_launches = 0;
    });
}

int az_mcts_profile(az_mcts *m, int enable)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        if (enable) {
            m->ev_select.allocate(AZ_PROFILE_MAX);
            m->ev_backprop.allocate(AZ_PROFILE_MAX);
        }
        m->profiling = enable != 0;
        m->profile_stride = enable > 1 ? enable : 1;
        m->profile_seen[0] = m->profile_seen[1] = 0;
    });
}

const char *az_mcts_timed_select_kernel(az_mcts *m) { return m ? m->timed_select_kernel : ""; }

int az_mcts_profile_read(az_mcts *m, double out_ms[2], int64_t out_launches[2])
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        m->ev_select.read(out_ms[0], out_launches[0]);
        m->ev_backprop.read(out_ms[1], out_launches[1]);
    });
}

int az_rng_gamma_selftest(uint32_t seed, float alpha, int count, float *out)
{
    az::HostRng r;
    r.seed(seed);
    r.gamma_fill(alpha, out, count);
    return AZ_OK;
}

}  // extern "C"
