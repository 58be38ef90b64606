// include/blaze.hpp's PoseidonClient against the C ABI: builds with -Wall -Werror; without a device it reports FileError (kind 7).
// usage: poseidon_host_example <instruction.csv> <height>
#include <cstdio>
#include <cstdlib>

#include "blaze.hpp"

using namespace ingo_blaze;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        PoseidonClient poseidon(Hash::Poseidon, DriverClient(0, DriverConfig::driver_client_cfg(CardType::MI355X)));
        const uint32_t h = uint32_t(atoi(argv[2]));
        poseidon.initialize(PoseidonInitializeParameters{h, TreeMode::TreeC, argv[1]});
        std::vector<uint8_t> element(32, 0);
        for (uint32_t i = 0; i < 11 * num_of_elements_in_base_layer(h); ++i) {
            element[0] = uint8_t(i);
            poseidon.set_data(element);
        }
        const auto res = poseidon.result(num_of_elements_oct_tree(h)).value();
        printf("%zu records, last (layer %u, id %u), %u pending\n", res.size(), res.back().layer_id, res.back().hash_id, poseidon.get_num_of_pending_results());
        return res.size() == num_of_elements_oct_tree(h) ? 0 : 3;
    } catch (const DriverClientError& e) {
        fprintf(stderr, "DriverClientError kind %d: %s\n", int(e.kind), e.what());
        return 1;
    }
}
