// gol_host.hpp -- native (C++17) host mirror of the reference's F# grid/generation interface, on top of
// the C ABI (gol.h).  The reference is compiled .NET code; this is its compiled-language counterpart,
// header-only, with the same names, argument meanings and error behaviour as the F# it mirrors:
//
//   Grid, Location, UpdateView, applyGrid   GameOfLife/GameOfLife/GameOfLifeLogic.fs:5-35
//   UpdateAgent (render agent)              GameOfLifeUI.fs:13-35 (GameofLife.fs:42-64): Reset starts a new
//                                           dictionary, each Update inserts, a full dictionary fills the Gray8
//                                           pixels[x + y*size] (128 / 0) and hands over the frame
//   Board                                   replaces the W*H cell agents (GameOfLifeLogic.fs:39-71)
//   run() -> GameOfLife (IDisposable)       GameOfLifeDriver.fs:13-41: seeded board, updateView = one tick =
//                                           UpdateView.Reset + one generation + the W*H Update posts (or one
//                                           rendered frame), optional timer (L38-40)
//
// Errors: the F# code fails with exceptions (failwith); every failing C-ABI call here throws gol::Error
// carrying gol_last_error().  The reference has no error channel for its agents.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <map>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "gol.h"

namespace gol {

struct Error : std::runtime_error {
    int code;
    Error(const std::string& what, int c) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, const char* what) {
    if (rc != GOL_OK) throw Error(std::string(what) + " failed (" + std::to_string(rc) + "): " + gol_last_error(), rc);
}

// ---------------------------------------------------------------- GameOfLifeLogic.fs:5-35
constexpr int size = 100;                        // L5
struct Grid {                                    // L6
    int Width;
    int Height;
};
constexpr Grid grid{size, size};                 // L8
constexpr int gridProduct = size * size;         // L7
struct Location {                                // L10-11 ([<Struct>] {x; y})
    int x;
    int y;
    bool operator<(const Location& o) const { return x != o.x ? x < o.x : y < o.y; }
    bool operator==(const Location& o) const { return x == o.x && y == o.y; }
};
struct UpdateView {                              // L32-35: Reset | Update of bool * Location
    enum Kind { Reset, Update } kind;
    bool alive = false;
    Location location{0, 0};
    static UpdateView reset() { return {Reset, false, {0, 0}}; }
    static UpdateView update(bool a, Location l) { return {Update, a, l}; }
};
template <class F>
void applyGrid(F&& f, Grid g = grid) {           // L13-15: x outer, y inner
    for (int x = 0; x < g.Width; x++)
        for (int y = 0; y < g.Height; y++) f(x, y);
}

// ---------------------------------------------------------------- a batch of small boards (gol.h gol_batch_*)
// `count` independent boards of one single-wave geometry, one wavefront per board, all stepped by one launch: the
// ensemble the reference samples one clock seed at a time (GameOfLifeDriver.fs:9-11).  Cells: boards back to back,
// cells[i*W*H + x + y*W].
class Batch {
   public:
    Batch(int64_t width, int64_t height, int64_t count, int boundary = GOL_TORUS) : w_(width), h_(height), n_(count) {
        check(gol_batch_create(width, height, boundary, count, &b_), "gol_batch_create");
    }
    ~Batch() {
        if (b_) gol_batch_destroy(b_);
    }
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;
    Batch(Batch&& o) noexcept : b_(std::exchange(o.b_, nullptr)), w_(o.w_), h_(o.h_), n_(o.n_) {}

    int64_t width() const { return w_; }
    int64_t height() const { return h_; }
    int64_t count() const { return n_; }
    Batch& seedDotnet(const std::vector<int32_t>& seeds, int mode = GOL_INIT_DOTNET_MOD2) {
        check(gol_batch_seed_dotnet(b_, seeds.data(), (int64_t)seeds.size(), mode), "gol_batch_seed_dotnet");
        return *this;
    }
    Batch& seedSplitmix(uint64_t seed) {
        check(gol_batch_seed_splitmix(b_, seed), "gol_batch_seed_splitmix");
        return *this;
    }
    Batch& clear() {
        check(gol_batch_clear(b_), "gol_batch_clear");
        return *this;
    }
    Batch& setCells(const std::vector<uint8_t>& cells, int64_t first = 0) {  // cells.size() / (W*H) boards
        check(gol_batch_set_cells(b_, first, (int64_t)cells.size() / (w_ * h_), cells.data(), (int64_t)cells.size()),
              "gol_batch_set_cells");
        return *this;
    }
    std::vector<uint8_t> getCells(int64_t first, int64_t n) const {
        std::vector<uint8_t> c(n > 0 ? (size_t)(n * w_ * h_) : 0);
        check(gol_batch_get_cells(b_, first, n, c.data(), (int64_t)c.size()), "gol_batch_get_cells");
        return c;
    }
    // the rule of every later step, stepTrace and cycles (B3/S23 until set): "B36/S23", "S23/B36" or "23/36"
    Batch& setRule(const std::string& rule) {
        int birth = 0, survive = 0;
        check(gol_rule_parse(rule.c_str(), &birth, &survive), "gol_rule_parse");
        return setRule(birth, survive);
    }
    Batch& setRule(int birth, int survive) {  // 9-bit masks, bit n = n live neighbours
        check(gol_ensemble_set_rule(b_, birth, survive), "gol_ensemble_set_rule");
        return *this;
    }
    std::string rule() const {  // canonical: "B36/S23"
        int birth = 0, survive = 0;
        char text[22];
        check(gol_ensemble_rule(b_, &birth, &survive), "gol_ensemble_rule");
        check(gol_rule_format(birth, survive, text, sizeof text), "gol_rule_format");
        return text;
    }
    // one rule per board (gol_ensemble_set_rules): count texts as setRule takes them, or count mask pairs; board i runs
    // under the i-th from now on, until another table or setRule.  rule() then throws where the boards differ
    Batch& setRules(const std::vector<std::string>& rules) {
        std::vector<int> birth(rules.size()), survive(rules.size());
        for (size_t i = 0; i < rules.size(); i++)
            check(gol_rule_parse(rules[i].c_str(), &birth[i], &survive[i]), "gol_rule_parse");
        return setRules(birth, survive);
    }
    Batch& setRules(const std::vector<int>& birth, const std::vector<int>& survive) {
        check(gol_ensemble_set_rules(b_, birth.data(), survive.data(),
                                     birth.size() == survive.size() ? (int64_t)birth.size() : -1),
              "gol_ensemble_set_rules");
        return *this;
    }
    std::vector<std::string> rules() const {  // canonical, one per board: the table, or count times the one rule
        std::vector<int> birth((size_t)n_), survive((size_t)n_);
        check(gol_ensemble_rules(b_, birth.data(), survive.data(), n_), "gol_ensemble_rules");
        std::vector<std::string> out((size_t)n_);
        char text[22];
        for (size_t i = 0; i < out.size(); i++) {
            check(gol_rule_format(birth[i], survive[i], text, sizeof text), "gol_rule_format");
            out[i] = text;
        }
        return out;
    }
    Batch& step(int64_t generations = 1) {
        check(gol_batch_step(b_, generations), "gol_batch_step");
        return *this;
    }
    // trace[t*count + i] = population of board i after generation every*(t + 1) of this call
    std::vector<uint32_t> stepTrace(int64_t generations, int64_t every = 1) {
        std::vector<uint32_t> t(generations > 0 && every > 0 ? (size_t)(generations / every * n_) : 0);
        check(gol_batch_step_trace(b_, generations, every, t.data(), (int64_t)t.size()), "gol_batch_step_trace");
        return t;
    }
    int64_t generation() const {
        int64_t g = 0;
        check(gol_batch_generation(b_, &g), "gol_batch_generation");
        return g;
    }
    std::vector<int64_t> populations() const {
        std::vector<int64_t> p((size_t)n_);
        check(gol_batch_populations(b_, p.data(), n_), "gol_batch_populations");
        return p;
    }
    std::vector<uint64_t> hashes() const {
        std::vector<uint64_t> p((size_t)n_);
        check(gol_batch_hashes(b_, p.data(), n_), "gol_batch_hashes");
        return p;
    }
    std::vector<uint8_t> renderGray8(int64_t board, uint8_t alive_value = 128) const {
        std::vector<uint8_t> p((size_t)(w_ * h_));
        check(gol_batch_render_gray8(b_, board, p.data(), w_, alive_value), "gol_batch_render_gray8");
        return p;
    }
    void synchronize() { check(gol_batch_synchronize(b_), "gol_batch_synchronize"); }
    // gol_ensemble_cycles: per board the transient, period and population of the cycle its current cells run into
    // within max_generations generations, (-1, 0, 0) where they do not; `steps` is the cost accounting gol.h describes
    struct Cycles {
        std::vector<int64_t> transient, period, population, steps;
    };
    Cycles cycles(int64_t max_generations) const {
        Cycles c;
        for (auto* v : {&c.transient, &c.period, &c.population, &c.steps}) v->resize((size_t)n_);
        check(gol_ensemble_cycles(b_, max_generations, c.transient.data(), c.period.data(), c.population.data(),
                                  c.steps.data(), n_),
              "gol_ensemble_cycles");
        return c;
    }

   private:
    gol_batch* b_ = nullptr;
    int64_t w_, h_, n_;
};

// ---------------------------------------------------------------- the board (replaces the cell agents)
class Board {
   public:
    // num_gpus > 1: row strips over devices 0..num_gpus-1 of this process (gol.h gol_create)
    Board(int64_t width, int64_t height, int boundary = GOL_TORUS, int tblock_k = 0, int num_gpus = 1)
        : w_(width), h_(height) {
        check(gol_create(width, height, boundary, num_gpus, tblock_k, &b_), "gol_create");
    }
    // explicit strip placement (gol_create_multi), e.g. {0, 0} runs two strips on one GPU
    Board(int64_t width, int64_t height, int boundary, int tblock_k, const std::vector<int>& devices)
        : w_(width), h_(height) {
        check(gol_create_multi(width, height, boundary, devices.data(), (int)devices.size(), tblock_k, 0, &b_),
              "gol_create_multi");
    }
    ~Board() {
        if (b_) gol_destroy(b_);
    }
    Board(const Board&) = delete;
    Board& operator=(const Board&) = delete;
    Board(Board&& o) noexcept : b_(std::exchange(o.b_, nullptr)), w_(o.w_), h_(o.h_) {}

    int64_t width() const { return w_; }
    int64_t height() const { return h_; }
    Board& seedDotnet(int32_t seed, int mode = GOL_INIT_DOTNET_MOD2) {
        check(gol_seed_dotnet(b_, seed, mode), "gol_seed_dotnet");
        return *this;
    }
    Board& setCells(const std::vector<uint8_t>& cells) {
        check(gol_set_cells(b_, cells.data(), (int64_t)cells.size()), "gol_set_cells");
        return *this;
    }
    Board& placeRle(const std::string& rle, int64_t x, int64_t y) {
        check(gol_place_rle(b_, rle.c_str(), x, y), "gol_place_rle");
        return *this;
    }
    // The rule of every later step ("B36/S23", "S23/B36", "23/36"; B3/S23 until set).  A property of the handle: the
    // setters and snapshots neither change nor carry it.  Boards on several GPUs take B3/S23 only.
    Board& setRule(const std::string& rule) {
        int birth = 0, survive = 0;
        check(gol_rule_parse(rule.c_str(), &birth, &survive), "gol_rule_parse");
        return setRule(birth, survive);
    }
    Board& setRule(int birth, int survive) {  // 9-bit masks, bit n = n live neighbours
        check(gol_set_rule(b_, birth, survive), "gol_set_rule");
        return *this;
    }
    std::string rule() const {  // canonical: "B36/S23"
        int birth = 0, survive = 0;
        char text[22];
        check(gol_rule(b_, &birth, &survive), "gol_rule");
        check(gol_rule_format(birth, survive, text, sizeof text), "gol_rule_format");
        return text;
    }
    // Generations rules ("B2/S345/4", "B2/S/C3"; two fields: two states): nstates 2..8 states per cell, the alive
    // cells where they were, state bytes through setStates / getStates.  Boards on several GPUs stay at two states.
    Board& setGenerationsRule(const std::string& rule) {
        int birth = 0, survive = 0, nstates = 2;
        check(gol_generations_parse(rule.c_str(), &birth, &survive, &nstates), "gol_generations_parse");
        check(gol_set_generations_rule(b_, birth, survive, nstates), "gol_set_generations_rule");
        return *this;
    }
    int nstates() const {
        int birth = 0, survive = 0, n = 2;
        check(gol_generations_rule(b_, &birth, &survive, &n), "gol_generations_rule");
        return n;
    }
    Board& setStates(const std::vector<uint8_t>& states) {  // states[x + y*W], each below nstates()
        check(gol_set_states(b_, states.data(), (int64_t)states.size()), "gol_set_states");
        return *this;
    }
    std::vector<uint8_t> getStates() const {
        std::vector<uint8_t> s((size_t)(w_ * h_));
        check(gol_get_states(b_, s.data(), (int64_t)s.size()), "gol_get_states");
        return s;
    }
    Board& step(int64_t generations = 1) {
        check(gol_step(b_, generations), "gol_step");
        return *this;
    }
    std::vector<uint8_t> getCells() const {  // cells[x + y*W]
        std::vector<uint8_t> c((size_t)(w_ * h_));
        check(gol_get_cells(b_, c.data(), (int64_t)c.size()), "gol_get_cells");
        return c;
    }
    std::vector<uint8_t> renderGray8(uint8_t alive_value = 128) const {
        std::vector<uint8_t> p((size_t)(w_ * h_));
        check(gol_render_gray8(b_, p.data(), w_, alive_value), "gol_render_gray8");
        return p;
    }
    // A zoomed or panned view (gol.h gol_view): counts[i + j*out_w] live cells of pixel (i, j) ...
    std::vector<uint32_t> viewCounts(const gol_view& v) const {
        std::vector<uint32_t> c(v.out_w > 0 && v.out_h > 0 ? (size_t)(v.out_w * v.out_h) : 0);
        check(gol_view_counts(b_, &v, c.data()), "gol_view_counts");
        return c;
    }
    // ... and its Gray8 frame, pixels[i + j*out_w] (GOL_VIEW_ANY | GOL_VIEW_DENSITY)
    std::vector<uint8_t> renderView(const gol_view& v, int mode = GOL_VIEW_ANY, uint8_t alive_value = 128) const {
        std::vector<uint8_t> p(v.out_w > 0 && v.out_h > 0 ? (size_t)(v.out_w * v.out_h) : 0);
        check(gol_render_view(b_, &v, mode, alive_value, p.data(), v.out_w), "gol_render_view");
        return p;
    }
    int64_t generation() const {
        int64_t g = 0;
        check(gol_generation(b_, &g), "gol_generation");
        return g;
    }
    int64_t population() const {
        int64_t p = 0;
        check(gol_population(b_, &p), "gol_population");
        return p;
    }
    uint64_t hash() const {
        uint64_t h = 0;
        check(gol_hash(b_, &h), "gol_hash");
        return h;
    }
    gol_board* handle() const { return b_; }

   private:
    gol_board* b_ = nullptr;
    int64_t w_, h_;
};

// ---------------------------------------------------------------- GameOfLifeUI.fs:13-35 (headless)
class UpdateAgent {
   public:
    using FrameFn = std::function<void(const std::vector<uint8_t>&)>;
    explicit UpdateAgent(Grid g = grid, uint8_t alive_value = 128, FrameFn on_frame = nullptr)
        : grid_(g), alive_(alive_value), pixels_((size_t)g.Width * g.Height, 0), on_frame_(std::move(on_frame)) {}

    void post(const UpdateView& msg) {
        std::lock_guard<std::mutex> lk(mu_);
        if (msg.kind == UpdateView::Reset) {  // L20: a new Dictionary
            states_.clear();
            return;
        }
        states_[msg.location] = msg.alive;  // L22
        if ((int64_t)states_.size() == (int64_t)grid_.Width * grid_.Height) {  // L23
            for (const auto& kv : states_)  // L24-28: pixels[x + y*size]
                pixels_[(size_t)(kv.first.x + kv.first.y * grid_.Width)] = kv.second ? alive_ : 0;
            frame_locked();
        }
    }
    // fast path: one frame rendered on the GPU instead of W*H Update messages
    void postFrame(std::vector<uint8_t> pixels) {
        std::lock_guard<std::mutex> lk(mu_);
        pixels_ = std::move(pixels);
        frame_locked();
    }
    int64_t frames() const { return frames_; }
    uint8_t aliveValue() const { return alive_; }
    Grid gridSize() const { return grid_; }
    std::vector<uint8_t> pixels() const {
        std::lock_guard<std::mutex> lk(mu_);
        return pixels_;
    }

   private:
    void frame_locked() {  // L29-31: WritePixels on the UI thread
        frames_++;
        if (on_frame_) on_frame_(pixels_);
    }
    Grid grid_;
    uint8_t alive_;
    std::vector<uint8_t> pixels_;
    FrameFn on_frame_;
    std::map<Location, bool> states_;  // Dictionary(HashIdentity.Structural)
    mutable std::mutex mu_;
    std::atomic<int64_t> frames_{0};
};

// ---------------------------------------------------------------- GameOfLifeDriver.fs:13-41
class GameOfLife {  // what run() returns: IDisposable
   public:
    enum class Emit { Updates, Pixels };
    GameOfLife(Board board, UpdateAgent& agent, Emit emit) : board_(std::move(board)), agent_(agent), emit_(emit) {}
    ~GameOfLife() { Dispose(); }
    GameOfLife(const GameOfLife&) = delete;
    GameOfLife& operator=(const GameOfLife&) = delete;

    // L32-34: one tick = UpdateView.Reset, then one generation for every cell.  Ticks may re-enter from
    // the timer (L38-40): serialised here.
    void updateView() {
        std::lock_guard<std::mutex> lk(tick_);
        agent_.post(UpdateView::reset());
        board_.step(1);
        if (emit_ == Emit::Pixels) {
            agent_.postFrame(board_.renderGray8(agent_.aliveValue()));
            return;
        }
        const auto cells = board_.getCells();
        const Grid g = agent_.gridSize();
        applyGrid([&](int x, int y) { agent_.post(UpdateView::update(cells[(size_t)(x + y * g.Width)] != 0, {x, y})); },
                  g);
    }
    // L38-40: a timer calling updateView every period.  A failed tick stops the timer and is kept for
    // lastError() (an exception escaping the thread would terminate the process; the .NET timer handler of
    // the reference does not bring the process down either).
    void start(std::chrono::milliseconds period) {
        timer_ = std::thread([this, period] {
            std::unique_lock<std::mutex> lk(stop_mu_);
            while (!stop_cv_.wait_for(lk, period, [this] { return stop_; })) {
                lk.unlock();
                try {
                    updateView();
                } catch (...) {
                    lk.lock();
                    error_ = std::current_exception();
                    stop_ = true;
                    break;
                }
                lk.lock();
            }
        });
    }
    // the exception of the tick that stopped the timer, or nullptr
    std::exception_ptr lastError() {
        std::lock_guard<std::mutex> lk(stop_mu_);
        return error_;
    }
    void Dispose() {
        {
            std::lock_guard<std::mutex> lk(stop_mu_);
            stop_ = true;
        }
        stop_cv_.notify_all();
        if (timer_.joinable()) timer_.join();
    }
    Board& board() { return board_; }

   private:
    Board board_;
    UpdateAgent& agent_;
    Emit emit_;
    std::mutex tick_;
    std::thread timer_;
    std::exception_ptr error_;
    std::mutex stop_mu_;
    std::condition_variable stop_cv_;
    bool stop_ = false;
};

// L13-41.  `seed` replaces `int DateTime.Now.Ticks` (L10) so runs are reproducible; the board is seeded
// x outer / y inner with Random.Next() % 2 = 0 (L9-11,16-19).  period 0 = no timer (ticks by hand).
inline GameOfLife* run(UpdateAgent& agent, int32_t seed, int boundary = GOL_TORUS,
                       std::chrono::milliseconds period = std::chrono::milliseconds(0),
                       GameOfLife::Emit emit = GameOfLife::Emit::Updates, int tblock_k = 0) {
    const Grid g = agent.gridSize();
    Board b(g.Width, g.Height, boundary, tblock_k);
    b.seedDotnet(seed, GOL_INIT_DOTNET_MOD2);
    auto* game = new GameOfLife(std::move(b), agent, emit);
    if (period.count() > 0) game->start(period);
    return game;
}

}  // namespace gol
