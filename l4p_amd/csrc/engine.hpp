// Engine state shared by the translation units of libl4p_hip.so (the launcher prototypes: launchers.hpp, gemm.hpp).
#pragma once
#include <string>
#include <unordered_map>

#include "gemm.hpp"
#include "launchers.hpp"

struct Weight {
    const void* ptr;
    long long numel;
};

struct l4p_engine {
    int device = 0;
    int dtype = L4P_BF16;
    std::unordered_map<std::string, Weight> w;
    l4p_encoder_cfg enc{};
    int enc_tokens = 0;
    bool enc_set = false;

    const void* find(const std::string& key) const {
        auto it = w.find(key);
        return it == w.end() ? nullptr : it->second.ptr;
    }
};
