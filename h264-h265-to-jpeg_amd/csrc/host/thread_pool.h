// The host thread pool of an engine: workers that run one parallel_for at a time, the caller with them.
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

namespace h2j {

class ThreadPool {
public:
    // n workers; cpus: if non-empty, every worker runs on that CPU set (NUMA-local slice)
    explicit ThreadPool(int n, const std::vector<int>& cpus = std::vector<int>()) : stop_(false), gen_(0), pending_(0) {
        for (int i = 0; i < n; i++) workers_.emplace_back([this] { loop(); });
        if (!cpus.empty()) {
            cpu_set_t set;
            CPU_ZERO(&set);
            for (int c : cpus)
                if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &set);
            for (auto& t : workers_)
                if (pthread_setaffinity_np(t.native_handle(), sizeof(set), &set) == 0) pinned_ = true;
        }
    }
    bool pinned() const { return pinned_; }
    ~ThreadPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    int size() const { return static_cast<int>(workers_.size()); }
    // run f(i) for i in [0, n) on the pool (caller participates)
    void parallel_for(int n, const std::function<void(int)>& f) {
        if (n <= 0) return;
        if (workers_.empty() || n == 1) {
            for (int i = 0; i < n; i++) f(i);
            return;
        }
        std::atomic<int> next(0);
        auto body = [&]() {
            for (;;) {
                int i = next.fetch_add(1);
                if (i >= n) break;
                f(i);
            }
        };
        {
            std::lock_guard<std::mutex> g(m_);
            task_ = body;
            pending_ = static_cast<int>(workers_.size());
            gen_++;
        }
        cv_.notify_all();
        body();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        task_ = nullptr;
    }

private:
    void loop() {
        unsigned long seen = 0;
        for (;;) {
            std::function<void()> t;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                t = task_;
            }
            if (t) t();
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::function<void()> task_;
    bool pinned_ = false;
    bool stop_;
    unsigned long gen_;
    int pending_;
};

}  // namespace h2j
