// shard_plan_test.cpp — the host arithmetic of the shard's exchanges
// (sherman_amd/csrc/shard_plan.h) for every rank of a world at once: from a
// matrix C[r][p] (rank r routes C[r][p] keys to shard p) every rank builds
// its plan out of what it would see on its own -- its row, and the column
// the count exchange delivers -- and the P plans must fit together: what r
// sends p is what p expects from r, ranges do not overlap, totals are the
// sums of the tails.  A routed get sends its tails from a packed overflow
// list, a routed insert from inside the bucketed batch; both rules are
// checked.  Pure host code: no GPU, no library.  `make -C tests/native
// sanitize` builds and runs it with the address and undefined-behaviour
// sanitizers.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../sherman_amd/csrc/shard_plan.h"

using namespace shm::shard;

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++fails;                                              \
    }                                                       \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

using Matrix = std::vector<std::vector<uint64_t>>;

static uint64_t tail(uint64_t c, uint64_t cap) { return c > cap ? c - cap : 0; }

// what rank r holds after the first round: its own row, and the counts the
// peers sent it; its own word of the received counts was never exchanged
// (stale: anything), which the own-run rule must not read
template <class C>
static void seen_by(const Matrix& m, uint32_t r, std::vector<C>& sent, std::vector<C>& received) {
  const uint32_t P = (uint32_t)m.size();
  sent.assign(P, 0);
  received.assign(P, 0);
  for (uint32_t p = 0; p < P; ++p) {
    sent[p] = (C)m[r][p];
    received[p] = p == r ? (C)0x5A5A5A5Au : (C)m[p][r];
  }
}

// C: the count words' type (u32 in a get's cursor words, u64 in an insert's)
template <class C>
static void check_tails(const Matrix& m, uint64_t cap, TailsAt at) {
  const uint32_t P = (uint32_t)m.size();
  std::vector<ExchangePlan> plan;
  bool any = false;
  for (uint32_t r = 0; r < P; ++r) {
    std::vector<C> sent, received;
    seen_by(m, r, sent, received);
    plan.push_back(plan_tails(sent.data(), received.data(), P, r, cap, at));
    for (uint32_t p = 0; p < P; ++p) any = any || m[r][p] > cap;
  }
  for (uint32_t r = 0; r < P; ++r) {
    const ExchangePlan& x = plan[r];
    CHECK(x.scnt.size() == P && x.soff.size() == P && x.rcnt.size() == P && x.roff.size() == P);
    uint64_t ns = 0, nr = 0, run = 0;
    for (uint32_t p = 0; p < P; ++p) {
      // the pair agrees, a rank with itself included
      CHECK(x.scnt[p] == plan[p].rcnt[r]);
      CHECK(x.scnt[p] == tail(m[r][p], cap));
      CHECK(x.rcnt[p] == tail(m[p][r], cap));
      // received tails: packed in peer order
      CHECK(x.roff[p] == nr);
      if (at == TailsAt::kPacked) {
        CHECK(x.soff[p] == ns);
      } else {
        // behind the slot's worth of run p, inside run p, before run p + 1
        CHECK(x.soff[p] == run + cap);
        if (x.scnt[p]) CHECK(x.soff[p] + x.scnt[p] == run + m[r][p]);
      }
      run += m[r][p];
      ns += x.scnt[p];
      nr += x.rcnt[p];
    }
    CHECK(x.ns == ns && x.nr == nr);
    if (!any) {
      CHECK(x.ns == 0 && x.nr == 0);
      for (uint32_t p = 0; p < P; ++p) CHECK(x.scnt[p] == 0 && x.rcnt[p] == 0);
    }
  }
}

// counts known to both sides (a range scan's value totals, a rebalance's
// moves): plain prefix offsets
static void check_packed(const Matrix& m) {
  const uint32_t P = (uint32_t)m.size();
  std::vector<ExchangePlan> plan;
  for (uint32_t r = 0; r < P; ++r) {
    std::vector<uint64_t> send(P), recv(P);
    for (uint32_t p = 0; p < P; ++p) {
      send[p] = m[r][p];
      recv[p] = m[p][r];
    }
    plan.push_back(plan_packed(send.data(), recv.data(), P));
  }
  for (uint32_t r = 0; r < P; ++r) {
    const ExchangePlan& x = plan[r];
    uint64_t ns = 0, nr = 0;
    for (uint32_t p = 0; p < P; ++p) {
      CHECK(x.scnt[p] == m[r][p] && x.scnt[p] == plan[p].rcnt[r]);
      CHECK(x.soff[p] == ns && x.roff[p] == nr);
      ns += x.scnt[p];
      nr += x.rcnt[p];
    }
    CHECK(x.ns == ns && x.nr == nr);
    ExchangePlan y = x;
    y.skip(r);
    CHECK(y.scnt[r] == 0 && y.rcnt[r] == 0 && y.soff == x.soff && y.roff == x.roff);
    CHECK(y.ns == x.ns && y.nr == x.nr);
  }
}

static void check_all(const Matrix& m, uint64_t cap) {
  check_tails<uint32_t>(m, cap, TailsAt::kPacked);   // get_overflow
  check_tails<uint64_t>(m, cap, TailsAt::kInRuns);   // flush
  check_tails<uint64_t>(m, cap, TailsAt::kPacked);
  check_tails<uint32_t>(m, cap, TailsAt::kInRuns);
  check_packed(m);
}

static void check_slot_cap(uint64_t n, uint32_t P) {
  const uint64_t c = get_slot_cap(n, P);
  CHECK(c * P >= n);
  CHECK(c >= n / P + 256);
}

int main() {
  for (uint32_t P = 1; P <= 16; ++P) {
    for (uint64_t cap : {1ull, 64ull, 1000ull}) {
      // entries below, at and above the capacity, and empty runs
      for (int round = 0; round < 40; ++round) {
        Matrix m(P, std::vector<uint64_t>(P, 0));
        for (auto& row : m)
          for (uint64_t& c : row) {
            switch (rnd() % 6) {
              case 0: c = 0; break;
              case 1: c = rnd() % (cap + 1); break;
              case 2: c = cap - 1; break;
              case 3: c = cap; break;
              case 4: c = cap + 1; break;
              default: c = cap + 1 + rnd() % (8 * cap); break;
            }
          }
        check_all(m, cap);
      }
      // nothing past a slot
      for (int round = 0; round < 10; ++round) {
        Matrix m(P, std::vector<uint64_t>(P, 0));
        for (auto& row : m)
          for (uint64_t& c : row) c = rnd() % (cap + 1);
        check_all(m, cap);
      }
      // every key of every rank belongs to one shard
      for (uint32_t hot = 0; hot < P; ++hot) {
        Matrix m(P, std::vector<uint64_t>(P, 0));
        for (uint32_t r = 0; r < P; ++r) m[r][hot] = 8 * cap + r;
        check_all(m, cap);
      }
      check_all(Matrix(P, std::vector<uint64_t>(P, 0)), cap);
    }
    // the get slot holds a uniform batch's share: every n up to 2^16, then
    // a coprime stride and the powers of two with their neighbours up to 2^24
    for (uint64_t n = 0; n <= (1u << 16); ++n) check_slot_cap(n, P);
    for (uint64_t n = 1u << 16; n <= (1u << 24); n += 251) check_slot_cap(n, P);
    for (uint32_t b = 16; b <= 24; ++b)
      for (uint64_t n = (1ull << b) - 2; n <= (1ull << b) + 2 && n <= (1u << 24); ++n)
        check_slot_cap(n, P);
  }
  if (fails) {
    printf("shard_plan_test: %d checks failed\n", fails);
    return 1;
  }
  printf("shard_plan_test ok\n");
  return 0;
}
