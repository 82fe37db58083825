// aqc_keep.hpp — objects that are expensive to set up (the device decoders of .gz and .bz2 input: gigabytes of device buffers,
// page-locked stages, threads) kept for the life of the process.  Host only: no HIP header, so aqc_pipe.cpp and the .hip units
// share it.
//
// A Keep lives on the heap and is never destroyed: its destructor is deleted, so it cannot have static or automatic storage, and
// the one who holds it is a plain pointer — `Keep<K, T>* const g_x = new Keep<K, T>;`.  Nothing it keeps is destroyed at exit():
// a kept object's destructor would call HIP (hipFree, hipStreamDestroy) and aqc_host_free from a static destructor, in no fixed
// order against the HIP runtime's own tear-down and against the statics of other units (aqc_dev.hpp).  What is kept stays
// reachable through that pointer, and goes with the process.
#pragma once
#include <cstddef>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace aqc {

template <class Key, class T>
class Keep {
public:
    static constexpr size_t CAP = 16;       // objects that wait in it for their next user (give)
    ~Keep() = delete;
    // the object that waits under an equal key, removed from the keeper; null: there is none
    std::unique_ptr<T> take(const Key& key) {
        std::lock_guard<std::mutex> g(mu_);
        for (size_t i = 0; i < kept_.size(); ++i)
            if (kept_[i].first == key) {
                std::unique_ptr<T> obj = std::move(kept_[i].second);
                kept_.erase(kept_.begin() + (long)i);
                return obj;
            }
        return nullptr;
    }
    // `obj` waits for the next take(key) and null comes back — or, with CAP objects waiting, `obj` itself: the caller destroys it,
    // on its own thread and while the process is still whole
    std::unique_ptr<T> give(const Key& key, std::unique_ptr<T> obj) {
        std::lock_guard<std::mutex> g(mu_);
        if (!obj || kept_.size() >= CAP) return obj;
        kept_.emplace_back(key, std::move(obj));
        return nullptr;
    }
    // the one object of this key that everybody who asks shares, made by make() (a T*, null: it cannot be made, ask again) when
    // the first one asks.  It stays for the life of the process and take() never hands it out.
    template <class Make>
    T* lend(const Key& key, Make&& make) {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& e : lent_) if (e.first == key) return e.second.get();
        std::unique_ptr<T> made(make());
        if (!made) return nullptr;
        lent_.emplace_back(key, std::move(made));
        return lent_.back().second.get();
    }

private:
    std::mutex mu_;
    std::vector<std::pair<Key, std::unique_ptr<T>>> kept_, lent_;
};

}  // namespace aqc
