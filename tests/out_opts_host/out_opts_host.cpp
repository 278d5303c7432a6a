// The output-options module alone (tests/test_out_opts_grid.py builds this with AddressSanitizer and UBSan and runs
// it): csrc/host/out_opts.cpp is the only file of the project it links, which shows that the module needs no
// thread, no GPU call and no engine.  It reads the calls of a grid file (tests/out_opts_grid.py: `<call> -> <answer>`
// a line, the option struct as its int32 words) and prints every line with the module's own answer.
//   out_opts_host <grid file>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "out_opts.h"

// the first words of `w` as an item of option type T (the rest, if T is longer, 0)
template <typename T>
static T item(const std::vector<int32_t>& w) {
    T o;
    std::memset(&o, 0, sizeof(o));
    std::memcpy(&o, w.data(), std::min(sizeof(o), w.size() * sizeof(int32_t)));
    return o;
}

template <typename T>
static std::string window(int W, int H, int sei, const std::vector<int32_t>& words) {
    const T o = item<T>(words);
    int32_t win[4] = {0, 0, 0, 0};
    int ow = 0, oh = 0, orient = 0;
    const int rc = h2j::crop_window(W, H, &o, sei, win, &ow, &oh, &orient);
    if (rc) return std::to_string(rc);
    char buf[128];
    snprintf(buf, sizeof(buf), "%d %d %d %d %d %d %d %d", rc, orient, win[0], win[1], win[2], win[3], ow, oh);
    return buf;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char line[1024];
    while (fgets(line, sizeof(line), f)) {
        std::string call(line);
        const size_t arrow = call.find(" -> ");
        if (arrow == std::string::npos) return 3;
        call.resize(arrow);
        std::istringstream in(call);
        std::string name;
        in >> name;
        std::vector<int32_t> a;
        for (long long v; in >> v;) a.push_back(static_cast<int32_t>(v));
        std::string answer;
        if (name == "fit" && a.size() == 5) {
            int ow = 0, oh = 0;
            const int rc = h2j::fit_size(a[0], a[1], a[2], a[3], a[4], &ow, &oh);
            answer = rc ? std::to_string(rc) : "0 " + std::to_string(ow) + " " + std::to_string(oh);
        } else if (a.size() > 3) {
            const std::vector<int32_t> words(a.begin() + 3, a.end());
            if (name == "win1") answer = window<h2j_out_opts>(a[0], a[1], a[2], words);
            else if (name == "win2") answer = window<h2j_out_opts2>(a[0], a[1], a[2], words);
            else if (name == "win3") answer = window<h2j_out_opts3>(a[0], a[1], a[2], words);
            else if (name == "win4") answer = window<h2j_out_opts4>(a[0], a[1], a[2], words);
            else if (name == "win5") answer = window<h2j_out_opts5>(a[0], a[1], a[2], words);
            else if (name == "win6") answer = window<h2j_out_opts6>(a[0], a[1], a[2], words);
        }
        if (answer.empty()) return 3;
        printf("%s -> %s\n", call.c_str(), answer.c_str());
    }
    fclose(f);
    return 0;
}
