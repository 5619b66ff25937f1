// Stand-alone check of bn_host.hpp (the host bignum behind sec_apdp_verify_batch's exponents),
// built with -fsanitize=address,undefined by tests/test_native_bn_host.py.  Reads vectors that
// the Python test wrote from Python ints, one per line, numbers in hex:
//   mul a b r            a * b == r
//   sub a b r            a - b == r (a >= b)
//   cmp a b s            cmp(a, b) == s - 1 (s in 0, 1, 2)
//   mod a m r o f k      a mod m == r, and the division met at least o quotient estimates that
//                        reached the base, f corrections by the second divisor limb and k add-back
//                        steps
//   pos t hm1 r          pos_exp(t, hm1) == r
//   neg t hm1 r          neg_exp(t, hm1) == r
//   be nbytes a          store_be / load_be round trip at nbytes, and store_be refusing nbytes - 1
//                        when a needs all nbytes
// and requires that the vectors together took each of the three division branches.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bn_host.hpp"

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "%s:%d: line %d: failed: %s\n", __FILE__, __LINE__, g_line, #c); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

using sec::bnh::Limbs;
static int g_line = 0;

// the test's own hex parser, so load_be is checked and not assumed
static Limbs hex(const std::string &h)
{
    Limbs a((h.size() + 7) / 8, 0u);
    for (size_t i = 0; i < h.size(); ++i) {
        const char c = h[h.size() - 1 - i];
        const uint32_t v = c >= 'a' ? (uint32_t)(c - 'a' + 10) : (uint32_t)(c - '0');
        a[i / 8] |= v << (4 * (i % 8));
    }
    while (!a.empty() && a.back() == 0)
        a.pop_back();
    return a;
}

int main(int argc, char **argv)
{
    namespace bnh = sec::bnh;
    REQUIRE(argc == 2);
    std::ifstream in(argv[1]);
    REQUIRE(in.good());
    bnh::DivStats total;
    std::string line;
    int checked = 0;
    while (std::getline(in, line)) {
        ++g_line;
        std::istringstream ss(line);
        std::string op, a, b, r;
        ss >> op;
        if (op.empty())
            continue;
        if (op == "be") {
            size_t nbytes = 0;
            ss >> nbytes >> a;
            const Limbs x = hex(a);
            std::vector<uint8_t> buf(nbytes + 1, 0xAB);
            REQUIRE(bnh::store_be(x, buf.data(), nbytes));
            REQUIRE(buf[nbytes] == 0xAB);
            REQUIRE(bnh::cmp(bnh::load_be(buf.data(), nbytes), x) == 0);
            if (nbytes > 0 && buf[0] != 0) {  // all nbytes are needed: one fewer must be refused
                std::vector<uint8_t> small(nbytes, 0xCD);
                REQUIRE(!bnh::store_be(x, small.data(), nbytes - 1));
                REQUIRE(small[0] == 0xCD && small[nbytes - 1] == 0xCD);
            }
        } else {
            ss >> a >> b >> r;
            const Limbs x = hex(a), y = hex(b), want = hex(r);
            if (op == "mul") {
                REQUIRE(bnh::cmp(bnh::mul(x, y), want) == 0);
                REQUIRE(bnh::cmp(bnh::mul(y, x), want) == 0);
            } else if (op == "sub") {
                REQUIRE(bnh::cmp(bnh::sub(x, y), want) == 0);
            } else if (op == "cmp") {
                REQUIRE(bnh::cmp(x, y) == atoi(r.c_str()) - 1);
            } else if (op == "mod") {
                unsigned long long o = 0, f = 0, k = 0;
                ss >> o >> f >> k;
                bnh::DivStats st;
                REQUIRE(bnh::cmp(bnh::mod(x, y, &st), want) == 0);
                REQUIRE(st.qhat_overflow >= o && st.qhat_fix >= f && st.add_back >= k);
                REQUIRE(bnh::cmp(bnh::mod(x, y), want) == 0);
                total.qhat_overflow += st.qhat_overflow;
                total.qhat_fix += st.qhat_fix;
                total.add_back += st.add_back;
            } else if (op == "pos") {
                REQUIRE(bnh::cmp(bnh::pos_exp(x, y), want) == 0);
            } else if (op == "neg") {
                REQUIRE(bnh::cmp(bnh::neg_exp(x, y), want) == 0);
            } else {
                REQUIRE(!"unknown op");
            }
        }
        REQUIRE(!ss.fail());
        ++checked;
    }
    REQUIRE(checked > 0);
    REQUIRE(total.qhat_overflow > 0);
    REQUIRE(total.qhat_fix > 0);
    REQUIRE(total.add_back > 0);
    printf("native bn_host tests ok: %d vectors, qhat_overflow %llu, qhat_fix %llu, add_back %llu\n", checked,
           (unsigned long long)total.qhat_overflow, (unsigned long long)total.qhat_fix,
           (unsigned long long)total.add_back);
    return 0;
}
