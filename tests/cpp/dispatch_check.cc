// dispatch_check.cc — csrc/dispatch.h on the host: the precision, (dim, degree)
// and int-list visitors reach exactly the listed instantiations, refuse
// everything else with a runtime_error that names the caller, and pass the
// visitor's return value through.  Stand-alone (no HIP, no GPU).
#include "dispatch.h"

#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

using namespace gls;

static int failures = 0;

#define CHECK(cond)                                              \
  do                                                             \
    {                                                            \
      if (!(cond))                                               \
        {                                                        \
          std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
          ++failures;                                            \
        }                                                        \
    }                                                            \
  while (0)

// f() throws a runtime_error whose text contains every string of `needles`
template <typename F>
static bool
throws_with(F &&f, std::vector<const char *> needles)
{
  try
    {
      f();
    }
  catch (const std::runtime_error &e)
    {
      for (const char *n : needles)
        if (!std::strstr(e.what(), n))
          {
            std::printf("message \"%s\" lacks \"%s\"\n", e.what(), n);
            return false;
          }
      return true;
    }
  return false;
}

int
main()
{
  // precision: the matching type, the return value passed through
  CHECK(with_real(GLS_F64, [](auto t) { return sizeof(t); }) == 8);
  CHECK(with_real(GLS_F32, [](auto t) { return sizeof(t); }) == 4);
  CHECK(with_real(GLS_F64, [](auto t) { return std::is_same<decltype(t), double>::value; }));
  CHECK(with_real(GLS_F32, [](auto t) { return std::is_same<decltype(t), float>::value; }));
  int hits = 0;
  with_real(GLS_F32, [&](auto) { ++hits; }); // a void visitor
  CHECK(hits == 1);
  CHECK(throws_with([] { with_real(7, [](auto t) { return sizeof(t); }); }, {"precision", "7"}));

  // (dim, degree): each of the six pairs reaches its own tags, once
  const int pairs[6][2] = {{2, 1}, {2, 2}, {2, 3}, {3, 1}, {3, 2}, {3, 3}};
  for (const auto &p : pairs)
    {
      int  calls = 0;
      auto got   = with_dim_degree(p[0], p[1], "pair_check", [&](auto d, auto k) {
        ++calls;
        static_assert(std::is_same<decltype(d), std::integral_constant<int, decltype(d)::value>>::value,
                      "dim tag");
        return std::make_pair((int)decltype(d)::value, (int)decltype(k)::value);
      });
      CHECK(calls == 1 && got.first == p[0] && got.second == p[1]);
    }
  const int bad[4][2] = {{1, 2}, {4, 2}, {2, 0}, {3, 4}};
  for (const auto &p : bad)
    CHECK(throws_with([&] { with_dim_degree(p[0], p[1], "pair_check", [](auto, auto) { return 0; }); },
                      {"pair_check", "(dim, degree)"}));

  // capped at degree 2: the four Q1 / Q2 pairs pass, the Q3 pairs are refused
  for (const auto &p : pairs)
    {
      auto run = [&] {
        return with_dim_degree<2>(p[0], p[1], "capped_check", [](auto d, auto k) {
          static_assert(decltype(k)::value <= 2, "no Q3 instantiation under the cap");
          return 10 * decltype(d)::value + decltype(k)::value;
        });
      };
      if (p[1] <= 2)
        CHECK(run() == 10 * p[0] + p[1]);
      else
        CHECK(throws_with(run, {"capped_check", "(dim, degree)"}));
    }

  // int list: every listed value, nothing else
  for (int v : {0, 1, 2})
    CHECK((with_int<0, 1, 2>(v, "list_check", [](auto m) { return 100 + decltype(m)::value; })) ==
          100 + v);
  CHECK((with_int<5>(5, "list_check", [](auto m) { return (int)decltype(m)::value; })) == 5);
  CHECK(throws_with([] { with_int<0, 1>(2, "list_check", [](auto) { return 0; }); },
                    {"list_check", "2"}));
  CHECK(throws_with([] { with_int<0, 1>(-1, "list_check", [](auto) { return 0; }); },
                    {"list_check"}));
  // a flag, and a nested call
  CHECK((with_int<0, 1>(true, "flag", [](auto b) { return decltype(b)::value != 0; })));
  const int nested = with_int<1, 2>(2, "outer", [&](auto a) {
    return with_int<0, 1>(1, "inner", [&](auto b) {
      return with_real(GLS_F32, [&](auto t) {
        return (int)(1000 * decltype(a)::value + 100 * decltype(b)::value + sizeof(t));
      });
    });
  });
  CHECK(nested == 2104);

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
