// Stand-alone check of the sequential model of the multiplicity count
// (blitzar_amd/csrc/proof/multiplicities.h: the hash, the slot count, model_insert, model_find,
// model_count) on tables built to be awkward: clusters that wrap past the last slot, duplicate
// rows, misses that start inside a cluster and must walk to its end, and tables as full as the slot
// count allows.  Built twice by build(), plain and under the address / undefined-behaviour
// sanitizers; tests/test_multiplicities_host.py compares the two outputs with each other and with
// the Python model.  One line per case:
//   name m=<rows> slots=<S> table=<keys> first=<first slot of each table key> lookups=<keys>
//   multiplicities=<counts> misses=<count> longest_probe=<steps>
// keys in hex, most significant word first.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "blitzar_amd/csrc/proof/multiplicities.h"

using namespace bz;
using namespace bz::proof;

namespace {
lookup_key small(u64 x) { return lookup_key{{x, 0, 0, 0}}; }
lookup_key wide(u64 x) { return lookup_key{{x, ~x, x * 3, 0x0123456789ABCDEFull}}; }

// the next `count` keys make(x), x >= from, whose probe starts at `slot`
template <class Make>
std::vector<lookup_key> keys_at(u64 slot, u64 slots, u64 count, u64& from, Make make) {
  std::vector<lookup_key> out;
  while (out.size() < count) {
    const lookup_key key = make(from++);
    if (first_slot(key, slots) == slot) out.push_back(key);
  }
  return out;
}

void print_keys(const char* label, const std::vector<lookup_key>& keys) {
  std::printf(" %s=", label);
  for (size_t i = 0; i < keys.size(); ++i) {
    std::printf("%s%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64, i ? "," : "",
                keys[i].w[3], keys[i].w[2], keys[i].w[1], keys[i].w[0]);
  }
}

void run(const char* name, const std::vector<lookup_key>& table,
         const std::vector<lookup_key>& lookups) {
  const u64 m = table.size(), slots = slot_count(m);
  // exactly `slots` words: a probe that leaves the table is the sanitizer's to find
  std::vector<u32> slot_rows(slots);
  std::vector<u64> multiplicities(m);
  u64 misses = ~u64{0};
  const auto table_key = [&](u64 t) { return table[t]; };
  model_insert(slot_rows.data(), slots, m, table_key);
  model_count(multiplicities.data(), &misses, slot_rows.data(), slots, m, table_key,
              lookups.size(), [&](u64 i) { return lookups[i]; });
  // how far the longest probe of a table key walks: the cluster the case was built for
  u64 longest = 0;
  for (u64 t = 0; t < m; ++t) {
    u64 slot = first_slot(table[t], slots), steps = 0;
    while (slot_rows[slot] != kEmptySlot && !same_key(table[slot_rows[slot]], table[t])) {
      slot = (slot + 1) & (slots - 1);
      ++steps;
    }
    longest = steps > longest ? steps : longest;
  }
  std::printf("%s m=%" PRIu64 " slots=%" PRIu64, name, m, slots);
  print_keys("table", table);
  std::printf(" first=");
  for (u64 t = 0; t < m; ++t) std::printf("%s%" PRIu64, t ? "," : "", first_slot(table[t], slots));
  print_keys("lookups", lookups);
  std::printf(" multiplicities=");
  for (u64 t = 0; t < m; ++t) std::printf("%s%" PRIu64, t ? "," : "", multiplicities[t]);
  std::printf(" misses=%" PRIu64 " longest_probe=%" PRIu64 "\n", misses, longest);
}

template <class T> void append(std::vector<T>& to, const std::vector<T>& from) {
  to.insert(to.end(), from.begin(), from.end());
}
} // namespace

int main() {
  // the slot count and the workspace at the edges
  std::printf("slot_count");
  for (u64 m : {u64{0}, u64{1}, u64{2}, u64{3}, u64{4}, u64{5}, u64{1} << 28, (u64{1} << 28) + 1}) {
    std::printf(" %" PRIu64 ":%" PRIu64 ":%" PRIu64, m, slot_count(m),
                multiplicity_workspace_bytes(m));
  }
  std::printf("\n");
  // small consecutive integers spread: 4096 of them over 8192 slots leave no slot with more than 8
  {
    std::vector<u32> load(8192, 0);
    u32 worst = 0;
    for (u64 x = 0; x < 4096; ++x) {
      const u32 here = ++load[first_slot(small(x), 8192)];
      worst = here > worst ? here : worst;
    }
    std::printf("spread worst=%s\n", worst <= 8 ? "ok" : "clustered");
  }
  for (int kind = 0; kind < 2; ++kind) {
    const auto make = [&](u64 x) { return kind == 0 ? small(x) : wide(x); };
    const std::string suffix = kind == 0 ? "_small" : "_wide";
    u64 from = 1;
    {
      // m = 5, 16 slots: four keys that start at the last slot lie in 15, 0, 1, 2; a key that starts
      // at 0 is pushed to 3.  Misses that start at 15, 0 and 2 walk to slot 4; one starts at an
      // empty slot
      std::vector<lookup_key> table = keys_at(15, 16, 4, from, make);
      append(table, keys_at(0, 16, 1, from, make));
      std::vector<lookup_key> lookups = {table[3], table[4], table[0], table[3], table[4], table[4]};
      append(lookups, keys_at(15, 16, 2, from, make));
      append(lookups, keys_at(0, 16, 1, from, make));
      append(lookups, keys_at(2, 16, 1, from, make));
      append(lookups, keys_at(9, 16, 1, from, make));
      lookups.push_back(table[2]);
      run(("wrap" + suffix).c_str(), table, lookups);
    }
    {
      // every key twice or more, the first occurrences out of order with the copies
      const std::vector<lookup_key> k = keys_at(3, 16, 3, from, make);
      const std::vector<lookup_key> table = {k[0], k[1], k[0], k[0], k[2], k[1], k[2]};
      std::vector<lookup_key> lookups = {k[2], k[2], k[1], k[0], k[2], k[0]};
      append(lookups, keys_at(3, 16, 1, from, make));
      run(("duplicates" + suffix).c_str(), table, lookups);
    }
    {
      // 40 keys with one first slot among 128 slots: the last of them is 39 steps away; misses that
      // start at the head, in the middle and at the last slot of the cluster
      std::vector<lookup_key> table = keys_at(100, 128, 40, from, make);
      std::vector<lookup_key> lookups(5, table[39]);
      lookups.push_back(table[0]);
      append(lookups, keys_at(100, 128, 1, from, make));
      append(lookups, keys_at(120, 128, 2, from, make));
      append(lookups, keys_at(11, 128, 1, from, make)); // 100 + 39 - 128: the cluster's last slot
      append(lookups, keys_at(12, 128, 1, from, make)); // the slot behind it
      run(("cluster" + suffix).c_str(), table, lookups);
    }
    {
      // the smallest tables: 1 row in 2 slots, 2 rows in 4, all rows equal
      const std::vector<lookup_key> one = keys_at(1, 2, 1, from, make);
      std::vector<lookup_key> lookups = {one[0], one[0]};
      append(lookups, keys_at(1, 2, 1, from, make));
      append(lookups, keys_at(0, 2, 1, from, make));
      run(("one_row" + suffix).c_str(), one, lookups);
      std::vector<lookup_key> two = keys_at(3, 4, 2, from, make);
      lookups = {two[1], two[0], two[1]};
      append(lookups, keys_at(3, 4, 1, from, make));
      append(lookups, keys_at(0, 4, 1, from, make));
      run(("two_rows" + suffix).c_str(), two, lookups);
      run(("all_equal" + suffix).c_str(), std::vector<lookup_key>(9, one[0]),
          {one[0], two[0], one[0]});
      run(("no_lookups" + suffix).c_str(), two, {});
    }
  }
  return 0;
}
